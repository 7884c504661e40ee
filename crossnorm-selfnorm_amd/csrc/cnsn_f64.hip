// Host side of the float64 entry points of include/cnsn_hip.h (cnsn_*_f64): argument validation, launch shape, and the plain
// streaming launches of cnsn_f64_kernels.h.  No persistent grid, no barrier, no context: three or four launches per direction.
#include "../../include/cnsn_hip.h"
#include "cnsn_env.h"

#include <hip/hip_runtime.h>

#include "cnsn_f64_kernels.h"
#include "cnsn_host_plan.h"

using namespace cnsn;

namespace {

// 16-byte loads: two doubles where the plane (with crop boxes: the row, so that a vector stays inside one) is even.  Lanes per
// plane by the number of VECTORS as in pick_shape: a vector is 16 bytes in either, so the classes cover the same bytes.
Shape pick_shape_f64(int M, int Wd, bool boxed) {
    Shape s;
    s.vec = ((boxed ? Wd : M) % 2 == 0) ? 2 : 1;
    const int nvec = M / s.vec;
    s.lpp = nvec <= 32 ? 16 : (nvec <= 4096 ? 64 : 256);
    return s;
}

// call f(IntTag<VEC>, IntTag<LPP>)
template <typename F>
void dispatch_f64(Shape s, F&& f) {
    auto with_lpp = [&](auto vtag) {
        switch (s.lpp) {
            case 16: f(vtag, IntTag<16>{}); break;
            case 64: f(vtag, IntTag<64>{}); break;
            default: f(vtag, IntTag<256>{}); break;
        }
    };
    if (s.vec == 2)
        with_lpp(IntTag<2>{});
    else
        with_lpp(IntTag<1>{});
}

int check_tensor_f64(const void* p, int N, int C, int H, int W) {
    if (!p) return CNSN_E_NULL;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return CNSN_E_SHAPE;
    if ((int64_t)N * C > (int64_t)1 << 30 || (int64_t)H * W > (int64_t)1 << 30) return CNSN_E_SHAPE;
    if (((uintptr_t)p & 15u) != 0) return CNSN_E_ALIGN;
    return CNSN_OK;
}

struct PlanD {
    cnsn_problem_t pr;
    Box cb, sb;
    bool boxed;
    Shape shape;
    Geom geom;
    MidArgsD mid;
    size_t P;
};

// `sc` may be NULL for the size query alone (the scalars do not change a size)
int make_plan_f64(const cnsn_problem_t* prob, const cnsn_f64_scalars_t* sc, PlanD& pl) {
    if (!prob) return CNSN_E_NULL;
    if (prob->struct_bytes != (int32_t)sizeof(cnsn_problem_t)) return CNSN_E_STRUCT;
    if (sc && sc->struct_bytes != (int32_t)sizeof(cnsn_f64_scalars_t)) return CNSN_E_STRUCT;
    pl.pr = *prob;
    const cnsn_problem_t& p = pl.pr;
    if (p.dtype != CNSN_F64) return CNSN_E_DTYPE;
    if (p.layout != CNSN_LAYOUT_NCHW) return CNSN_E_UNSUPPORTED;
    if (p.N <= 0 || p.C <= 0 || p.H <= 0 || p.W <= 0) return CNSN_E_SHAPE;
    if ((int64_t)p.N * p.C > (int64_t)1 << 30 || (int64_t)p.H * p.W > (int64_t)1 << 30) return CNSN_E_SHAPE;
    bool hc = false, hs = false;
    pl.cb = Box{0, 0, p.H, p.W};
    pl.sb = pl.cb;
    if (p.cn_active) {
        int st = parse_box(p.content_box, p.H, p.W, pl.cb, hc);
        if (st) return st;
        st = parse_box(p.style_box, p.H, p.W, pl.sb, hs);
        if (st) return st;
    }
    pl.boxed = hc || hs;
    if (p.sn_active && p.sn_training && p.N < 2) return CNSN_E_BATCH;
    pl.shape = pick_shape_f64(p.H * p.W, p.W, pl.boxed);
    pl.geom = make_geom(p.N, p.C, p.H, p.W, pl.shape.vec, pl.cb, pl.sb);
    // the keep_first_read rule of make_plan: up to 512 MiB the first pass leaves the tensor in the caches for the second
    pl.geom.keep = ((size_t)p.N * p.C * p.H * p.W * 8 <= ((size_t)512 << 20)) ? 1 : 0;
    if (const char* e = knob(K_KEEP)) pl.geom.keep = e[0] == '1' ? 1 : (e[0] == '0' ? 0 : pl.geom.keep);
    pl.P = (size_t)p.N * p.C;
    MidArgsD& m = pl.mid;
    m.N = p.N;
    m.C = p.C;
    m.M = p.H * p.W;
    m.Mc = pl.cb.area();
    m.Ms = pl.sb.area();
    m.cn_active = p.cn_active ? 1 : 0;
    m.boxed = pl.boxed ? 1 : 0;
    m.sn_active = p.sn_active ? 1 : 0;
    m.sn_two = (p.sn_active && p.sn_two) ? 1 : 0;
    m.sn_training = p.sn_training ? 1 : 0;
    m.lam = (sc && p.cn_active) ? sc->lam : 0.0;
    m.eps_cn = sc ? sc->eps_cn : 0.0;
    m.eps_sn = sc ? sc->eps_sn : 0.0;
    m.eps_bn = sc ? sc->eps_bn : 0.0;
    m.momentum = sc ? sc->momentum : 0.0;
    m.inv_n = 1.0 / (double)p.N;
    m.unbias_n = p.N > 1 ? (double)p.N / ((double)p.N - 1.0) : 1.0;
    m.save_coefs = 0;
    return CNSN_OK;
}

size_t saved_doubles_f64(const PlanD& pl) { return (size_t)SV_ROWS * pl.P + 2 * (size_t)pl.pr.C; }
// workspace (bytes), all doubles: forward  = moments[6P] | saved fallback | coef[FC_ROWS*P]
//                                  backward = tmp[BT_ROWS*P] | sums[4P] | coef[BC_ROWS*P]
size_t workspace_bytes_f64(const PlanD& pl) {
    const size_t fwd = 8 * (6 * pl.P + saved_doubles_f64(pl) + (size_t)FC_ROWS * pl.P);
    const size_t bwd = 8 * (size_t)(BT_ROWS + 4 + BC_ROWS) * pl.P;
    return (fwd > bwd ? fwd : bwd) + 256;
}

bool gate_ok_f64(const cnsn_gate_f64_t* g) {
    return g && g->fc_weight && g->bn_weight && g->bn_bias && g->running_mean && g->running_var;
}
bool gate_grad_ok_f64(const cnsn_gate_grad_f64_t* g) { return g && g->d_fc_weight && g->d_bn_weight && g->d_bn_bias; }
GateDevD gate_dev_f64(const cnsn_gate_f64_t* g) {
    GateDevD d{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (g) d = GateDevD{g->fc_weight, g->bn_weight, g->bn_bias, g->running_mean, g->running_var, (long long*)g->num_batches_tracked};
    return d;
}
GateGradDevD gate_grad_dev_f64(const cnsn_gate_grad_f64_t* g) {
    GateGradDevD d{nullptr, nullptr, nullptr};
    if (g) d = GateGradDevD{g->d_fc_weight, g->d_bn_weight, g->d_bn_bias};
    return d;
}
// the gates a call needs are there and carry this library's struct sizes
int check_gates_f64(const cnsn_problem_t& p, const cnsn_gate_f64_t* g, const cnsn_gate_f64_t* f) {
    if (!p.sn_active) return CNSN_OK;
    if (!gate_ok_f64(g) || (p.sn_two && !gate_ok_f64(f))) return CNSN_E_NULL;
    if (g->struct_bytes != (int32_t)sizeof(cnsn_gate_f64_t)) return CNSN_E_STRUCT;
    if (p.sn_two && f->struct_bytes != (int32_t)sizeof(cnsn_gate_f64_t)) return CNSN_E_STRUCT;
    return CNSN_OK;
}
int check_gate_grads_f64(const cnsn_problem_t& p, const cnsn_gate_grad_f64_t* dg, const cnsn_gate_grad_f64_t* df) {
    if (!p.sn_active) return CNSN_OK;
    if (!gate_grad_ok_f64(dg) || (p.sn_two && !gate_grad_ok_f64(df))) return CNSN_E_NULL;
    if (dg->struct_bytes != (int32_t)sizeof(cnsn_gate_grad_f64_t)) return CNSN_E_STRUCT;
    if (p.sn_two && df->struct_bytes != (int32_t)sizeof(cnsn_gate_grad_f64_t)) return CNSN_E_STRUCT;
    return CNSN_OK;
}

// geometry of a stand-alone per-plane primitive
struct PlaneCall {
    Shape s;
    Geom g;
    int blocks;
    bool boxed;
};
int plane_call_f64(int N, int C, int H, int W, const int32_t* box, PlaneCall& pc) {
    Box cb;
    const int st = parse_box(box, H, W, cb, pc.boxed);
    if (st) return st;
    pc.s = pick_shape_f64(H * W, W, pc.boxed);
    pc.g = make_geom(N, C, H, W, pc.s.vec, cb, cb);
    pc.blocks = blocks_for(pc.g.P, pc.s.lpp);
    return CNSN_OK;
}

}  // namespace

extern "C" {

size_t cnsn_workspace_bytes_f64(const cnsn_problem_t* prob) {
    PlanD pl;
    if (make_plan_f64(prob, nullptr, pl) != CNSN_OK) return 0;
    return workspace_bytes_f64(pl);
}

int cnsn_forward_f64(const cnsn_problem_t* prob, const cnsn_f64_scalars_t* sc, const double* x, const int64_t* perm,
                     const int64_t* chan_perm, const cnsn_gate_f64_t* g, const cnsn_gate_f64_t* f, double* y, float* saved,
                     void* workspace, size_t workspace_bytes, void* stream_) {
    if (!sc) return CNSN_E_NULL;
    PlanD pl;
    int st = make_plan_f64(prob, sc, pl);
    if (st) return st;
    const cnsn_problem_t& p = pl.pr;
    if (!x || !y || !workspace) return CNSN_E_NULL;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)workspace) & 15u) != 0) return CNSN_E_ALIGN;
    if (p.cn_active && !perm) return CNSN_E_NULL;
    st = check_gates_f64(p, g, f);
    if (st) return st;
    if (workspace_bytes < workspace_bytes_f64(pl)) return CNSN_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;

    const size_t P = pl.P;
    double* mom = (double*)workspace;
    double* saved_d = saved ? (double*)saved : mom + 6 * P;
    double* coef = mom + 6 * P + saved_doubles_f64(pl);
    const int blocks = blocks_for(pl.geom.P, pl.shape.lpp);
    dispatch_f64(pl.shape, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        if (pl.boxed)
            plane_stats_f64_kernel<VEC, LPP, true><<<blocks, kBlock, 0, stream>>>(x, pl.geom, mom, nullptr, 0.0);
        else
            plane_stats_f64_kernel<VEC, LPP, false><<<blocks, kBlock, 0, stream>>>(x, pl.geom, mom, nullptr, 0.0);
    });
    mid_fwd_f64_kernel<<<p.C, kBlock, 0, stream>>>(pl.mid, mom, perm, chan_perm, gate_dev_f64(g), gate_dev_f64(f), coef, saved_d);
    const ApplyCoefD cf{coef + FC_A_IN * P, coef + FC_XR * P, coef + FC_B_IN * P, coef + FC_A_OUT * P, coef + FC_B_OUT * P};
    dispatch_f64(pl.shape, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        if (pl.boxed)
            apply_fwd_f64_kernel<VEC, LPP, true><<<blocks, kBlock, 0, stream>>>(x, y, pl.geom, cf);
        else
            apply_fwd_f64_kernel<VEC, LPP, false><<<blocks, kBlock, 0, stream>>>(x, y, pl.geom, cf);
    });
    return launch_status();
}

int cnsn_backward_f64(const cnsn_problem_t* prob, const cnsn_f64_scalars_t* sc, const double* grad_y, const double* x,
                      const int64_t* perm, const int64_t* chan_perm, const cnsn_gate_f64_t* g, const cnsn_gate_f64_t* f,
                      const float* saved, double* grad_x, const cnsn_gate_grad_f64_t* dg, const cnsn_gate_grad_f64_t* df,
                      void* workspace, size_t workspace_bytes, void* stream_) {
    if (!sc) return CNSN_E_NULL;
    PlanD pl;
    int st = make_plan_f64(prob, sc, pl);
    if (st) return st;
    const cnsn_problem_t& p = pl.pr;
    if (!grad_y || !x || !grad_x || !saved || !workspace) return CNSN_E_NULL;
    if ((((uintptr_t)x | (uintptr_t)grad_y | (uintptr_t)grad_x | (uintptr_t)workspace) & 15u) != 0) return CNSN_E_ALIGN;
    if (p.cn_active && !perm) return CNSN_E_NULL;
    st = check_gates_f64(p, g, f);
    if (st) return st;
    st = check_gate_grads_f64(p, dg, df);
    if (st) return st;
    if (workspace_bytes < workspace_bytes_f64(pl)) return CNSN_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;

    const size_t P = pl.P;
    double* tmp = (double*)workspace;
    double* sums = tmp + BT_ROWS * P;
    double* coef = sums + 4 * P;
    const double* saved_d = (const double*)saved;
    const double* mu_c = saved_d + (size_t)SV_MU_C * p.N;  // rows of `saved` (shift_stride 0)
    const double* mu_o = pl.boxed ? saved_d + (size_t)SV_MU_O * p.N : nullptr;
    const int blocks = blocks_for(pl.geom.P, pl.shape.lpp);
    dispatch_f64(pl.shape, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        if (pl.boxed)
            bwd_reduce_f64_kernel<VEC, LPP, true><<<blocks, kBlock, 0, stream>>>(grad_y, x, pl.geom, mu_c, mu_o, 0, sums);
        else
            bwd_reduce_f64_kernel<VEC, LPP, false><<<blocks, kBlock, 0, stream>>>(grad_y, x, pl.geom, mu_c, nullptr, 0, sums);
    });
    mid_bwd_a_f64_kernel<<<p.C, kBlock, 0, stream>>>(pl.mid, sums, saved_d, perm, chan_perm, gate_dev_f64(g), gate_dev_f64(f),
                                                     gate_grad_dev_f64(dg), gate_grad_dev_f64(df), tmp, coef);
    if (pl.mid.cn_active)  // (without CrossNorm mid_bwd_a has written the coefficients itself)
        mid_bwd_b_f64_kernel<<<(int)((P + kBlock - 1) / kBlock), kBlock, 0, stream>>>(pl.mid, saved_d, tmp, coef);
    dispatch_f64(pl.shape, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        if (pl.boxed)
            apply_bwd_f64_kernel<VEC, LPP, true><<<blocks, kBlock, 0, stream>>>(grad_y, x, grad_x, pl.geom, coef);
        else
            apply_bwd_f64_kernel<VEC, LPP, false><<<blocks, kBlock, 0, stream>>>(grad_y, x, grad_x, pl.geom, coef);
    });
    return launch_status();
}

int cnsn_plane_stats_f64(const double* x, int N, int C, int H, int W, const int32_t* box, double eps, double* mean_std,
                         void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    if (!mean_std) return CNSN_E_NULL;
    PlaneCall pc;
    st = plane_call_f64(N, C, H, W, box, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    dispatch_f64(pc.s, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        if (pc.boxed)
            plane_stats_f64_kernel<VEC, LPP, true><<<pc.blocks, kBlock, 0, stream>>>(x, pc.g, nullptr, mean_std, eps);
        else
            plane_stats_f64_kernel<VEC, LPP, false><<<pc.blocks, kBlock, 0, stream>>>(x, pc.g, nullptr, mean_std, eps);
    });
    return launch_status();
}

int cnsn_plane_stats_backward_f64(const double* x, int N, int C, int H, int W, const int32_t* box, const double* mean,
                                  const double* std, const double* dmean, const double* dstd, double* dx, void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    if (!mean || !std || !dmean || !dstd || !dx) return CNSN_E_NULL;
    if (((uintptr_t)dx & 15u) != 0) return CNSN_E_ALIGN;
    PlaneCall pc;
    st = plane_call_f64(N, C, H, W, box, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    dispatch_f64(pc.s, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        if (pc.boxed)
            plane_stats_bwd_f64_kernel<VEC, LPP, true><<<pc.blocks, kBlock, 0, stream>>>(x, dx, pc.g, mean, std, dmean, dstd);
        else
            plane_stats_bwd_f64_kernel<VEC, LPP, false><<<pc.blocks, kBlock, 0, stream>>>(x, dx, pc.g, mean, std, dmean, dstd);
    });
    return launch_status();
}

int cnsn_plane_affine_f64(const double* x, int N, int C, int H, int W, const double* scale, const double* shift, double* y,
                          void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    if (!scale || !shift || !y) return CNSN_E_NULL;
    if (((uintptr_t)y & 15u) != 0) return CNSN_E_ALIGN;
    PlaneCall pc;
    st = plane_call_f64(N, C, H, W, nullptr, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    const ApplyCoefD cf{scale, nullptr, shift, nullptr, nullptr};
    dispatch_f64(pc.s, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        apply_fwd_f64_kernel<VEC, LPP, false><<<pc.blocks, kBlock, 0, stream>>>(x, y, pc.g, cf);
    });
    return launch_status();
}

int cnsn_plane_dot_f64(const double* gr, const double* x, int N, int C, int H, int W, double* sums, void* stream_) {
    int st = check_tensor_f64(x, N, C, H, W);
    if (st) return st;
    st = check_tensor_f64(gr, N, C, H, W);
    if (st) return st;
    if (!sums) return CNSN_E_NULL;
    PlaneCall pc;
    st = plane_call_f64(N, C, H, W, nullptr, pc);
    if (st) return st;
    hipStream_t stream = (hipStream_t)stream_;
    dispatch_f64(pc.s, [&](auto vt, auto lt) {
        constexpr int VEC = decltype(vt)::value, LPP = decltype(lt)::value;
        bwd_reduce_f64_kernel<VEC, LPP, false><<<pc.blocks, kBlock, 0, stream>>>(gr, x, pc.g, nullptr, nullptr, 1, sums);
    });
    return launch_status();
}

}  // extern "C"
