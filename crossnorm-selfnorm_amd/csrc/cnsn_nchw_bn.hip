// BatchNorm2d (+ add) + ReLU on NCHW tensors in two ordinary launches per direction (cnsn_nchw_bn_kernels.h): host side and the
// C ABI entry points (include/cnsn_hip.h, ABI 9, added in round 12).  The descriptor and its checks are those of the
// channels-last entry points (cnsn_nhwc_bn.hip); nothing here asks a switch, the resident health or a context.
#include "../../include/cnsn_hip.h"
#include "cnsn_nchw_bn_kernels.h"
#include "cnsn_nhwc_fused_host.h"

namespace cnsn {

using namespace nhwc_host;

namespace {

constexpr int kNchwTileBytes = 64 << 10;  // a tile of a large channel: 64 KiB of the tensor, 16 vectors per thread
constexpr int kNchwWorkgroups = 1024;     // workgroups the geometry aims at where the tensor has them: four per compute unit
constexpr int kNchwMaxTiles = 4096;       // tiles of a channel at most (every workgroup of launch 2 adds its channel's partials)

int nchw_parse(const cnsn_bn_act_t* d) {
    const int st = parse_desc_head(d);
    return st ? st : parse_bn_tail(d->bn);
}

long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// Elements of a tile: the channel cut into as many tiles as give the grid kNchwWorkgroups workgroups, between one vector per
// thread and kNchwTileBytes, more where a channel would otherwise have more than kNchwMaxTiles tiles.  A plane of two tiles or
// more is cut into equal ranges of whole vectors, one instance per tile; smaller planes go whole, as many instances per tile as
// fit, spread evenly.  A pure function of the shape and the element size — the same for both directions.
NchwBnGeom nchw_geom(const cnsn_bn_act_t& d) {
    const int vec = vec_of(d.dtype);
    const long long P = (long long)d.H * d.W, E = (long long)d.N * P;
    long long tile = E / ceil_div(kNchwWorkgroups, d.C);
    const long long tmin = (long long)kBlock * vec, tmax = kNchwTileBytes / elem_bytes(d.dtype);
    tile = tile < tmin ? tmin : (tile > tmax ? tmax : tile);
    if (tile < ceil_div(E, kNchwMaxTiles)) tile = ceil_div(E, kNchwMaxTiles);
    NchwBnGeom g{};
    g.N = d.N, g.C = d.C, g.P = (int)P;
    if (P >= 2 * tile) {
        const long long spp = ceil_div(P, tile);
        g.epr = (int)(ceil_div(ceil_div(P, spp), vec) * vec);
        g.spp = (int)ceil_div(P, g.epr);
        g.ipt = 1;
    } else {
        long long ipt = tile / P < 1 ? 1 : (tile / P > d.N ? d.N : tile / P);
        g.ipt = (int)ceil_div(d.N, ceil_div(d.N, ipt));
        g.epr = (int)P;
        g.spp = 1;
    }
    g.tpc = (int)ceil_div(d.N, g.ipt) * g.spp;
    return g;
}

// the index range: every count and the grid in 32 bits
bool nchw_shape_ok(const cnsn_bn_act_t& d) {
    const long long lim = (long long)1 << 31;  // (checked factor by factor: no product of two values below 2^31 overflows)
    const long long nh = (long long)d.N * d.H;
    if (nh >= lim || nh * d.W >= lim || nh * d.W * d.C >= lim) return false;
    return (long long)d.C * nchw_geom(d).tpc < lim;
}

bool nchw_ok(const cnsn_bn_act_t& d, bool backward) {
    if (!nchw_shape_ok(d)) return false;
    if (!d.bn.training) return !backward;
    return (long long)d.N * d.H * d.W >= 2;
}

// part [C][tpc][2]
struct NchwWs { float* part; size_t bytes; };
NchwWs nchw_layout(const NchwBnGeom& g, void* workspace) {
    Carver c(workspace);
    return {c.take((size_t)g.C * g.tpc * 2 * 4), c.bytes()};
}

NchwBnArgs nchw_args(const cnsn_bn_act_t& d, const NchwBnGeom& g, void* workspace) {
    NchwBnArgs a{};
    a.g = g;
    a.relu = d.relu ? 1 : 0;
    a.bn = bn_head_dev(d.bn);
    set_bn_count(a, (double)d.N * g.P);
    a.part = nchw_layout(g, workspace).part;
    return a;
}

int nchw_forward(const cnsn_bn_act_t& d, const void* x, const void* addend, void* y, float* saved, void* workspace,
                 hipStream_t stream) {
    const NchwBnGeom g = nchw_geom(d);
    const unsigned grid = (unsigned)g.C * (unsigned)g.tpc;
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(d.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        with_flag(addend != nullptr, [&](auto at) {
            constexpr bool ADD = decltype(at)::value;
            if (!d.bn.training) {
                nchw_bnact_eval_kernel<T, VEC, ADD><<<grid, kBlock, 0, stream>>>(g, bn_head_dev(d.bn, false), d.relu ? 1 : 0, (const T*)x,
                                                                                 (const T*)addend, (T*)y);
                status = launch_status();
                return;
            }
            NchwBnArgs a = nchw_args(d, g, workspace);
            a.stat = saved;
            nchw_bnact_fwd_stats_kernel<T, VEC><<<grid, kBlock, 0, stream>>>(a, (const T*)x);
            status = launch_status();
            if (status != CNSN_OK) return;
            nchw_bnact_fwd_apply_kernel<T, VEC, ADD><<<grid, kBlock, 0, stream>>>(a, (const T*)x, (const T*)addend, (T*)y);
            status = launch_status();
        });
    });
    return status;
}

int nchw_backward(const cnsn_bn_act_t& d, const void* gy, const void* x, const void* addend, const float* saved, void* dx,
                  void* d_addend, float* d_w, float* d_b, void* workspace, hipStream_t stream) {
    const NchwBnGeom g = nchw_geom(d);
    const unsigned grid = (unsigned)g.C * (unsigned)g.tpc;
    NchwBnArgs a = nchw_args(d, g, workspace);
    a.saved = saved;
    a.d_w = d_w;
    a.d_b = d_b;
    const bool add = d.relu && addend;  // (without the ReLU the addend's gradient is grad_y itself: nothing to read or write)
    int status = CNSN_E_UNSUPPORTED;
    dispatch_t(d.dtype, [&](auto tt, auto vt) {
        using T = typename decltype(tt)::type;
        constexpr int VEC = decltype(vt)::value;
        with_flag(add, [&](auto at) {
            constexpr bool ADD = decltype(at)::value;
            nchw_bnact_bwd_stats_kernel<T, VEC, ADD><<<grid, kBlock, 0, stream>>>(a, (const T*)gy, (const T*)x, (const T*)addend);
            status = launch_status();
            if (status != CNSN_OK) return;
            nchw_bnact_bwd_apply_kernel<T, VEC, ADD><<<grid, kBlock, 0, stream>>>(a, (const T*)gy, (const T*)x, (const T*)addend,
                                                                                  (T*)dx, (T*)d_addend);
            status = launch_status();
        });
    });
    return status;
}

}  // namespace
}  // namespace cnsn

using namespace cnsn;

extern "C" {

int cnsn_bn_act_nchw_plan(const cnsn_bn_act_t* desc, int has_addend, int backward) {
    (void)has_addend;  // (the addend changes the tensor passes, not whether the launches apply)
    const int st = nchw_parse(desc);
    if (st) return st;
    return nchw_ok(*desc, backward != 0) ? 1 : 0;
}

size_t cnsn_bn_act_nchw_workspace_bytes(const cnsn_bn_act_t* desc) {
    if (nchw_parse(desc) != CNSN_OK || !nchw_shape_ok(*desc)) return 0;
    return nchw_layout(nchw_geom(*desc), nullptr).bytes;
}

int cnsn_bn_act_nchw_geometry(const cnsn_bn_act_t* desc, int backward, int32_t out[4]) {
    const int st = nchw_parse(desc);
    if (st) return st;
    if (!out) return CNSN_E_NULL;
    if (!nchw_ok(*desc, backward != 0)) return CNSN_E_UNSUPPORTED;
    const NchwBnGeom g = nchw_geom(*desc);
    out[0] = g.tpc, out[1] = g.ipt, out[2] = g.epr, out[3] = kBlock;
    return CNSN_OK;
}

int cnsn_forward_bn_act_nchw(const cnsn_bn_act_t* desc, const void* x, const void* addend, void* y, float* saved, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const int st = nchw_parse(desc);
    if (st) return st;
    const cnsn_bn_act_t& d = *desc;
    if (!nchw_ok(d, false)) return CNSN_E_UNSUPPORTED;
    if (!x || !y || !workspace) return CNSN_E_NULL;
    if (!d.bn.weight || !d.bn.bias || !d.bn.running_mean || !d.bn.running_var) return CNSN_E_NULL;
    if (!aligned16(x) || !aligned16(y) || !aligned16(workspace) || (addend && !aligned16(addend))) return CNSN_E_UNSUPPORTED;
    if (workspace_bytes < nchw_layout(nchw_geom(d), nullptr).bytes) return CNSN_E_WORKSPACE;
    return nchw_forward(d, x, addend, y, saved, workspace, (hipStream_t)stream);
}

int cnsn_backward_bn_act_nchw(const cnsn_bn_act_t* desc, const void* grad_y, const void* x, const void* addend,
                              const float* saved, void* grad_x, void* grad_addend, float* d_weight, float* d_bias, void* workspace,
                              size_t workspace_bytes, void* stream) {
    const int st = nchw_parse(desc);
    if (st) return st;
    const cnsn_bn_act_t& d = *desc;
    if (!nchw_ok(d, true)) return CNSN_E_UNSUPPORTED;
    if (!grad_y || !x || !saved || !grad_x || !workspace || !d.bn.weight || !d.bn.bias) return CNSN_E_NULL;
    if (d.relu && addend && !grad_addend) return CNSN_E_NULL;
    if (!aligned16(grad_y) || !aligned16(x) || !aligned16(grad_x) || !aligned16(workspace) || (addend && !aligned16(addend)) ||
        (grad_addend && !aligned16(grad_addend)))
        return CNSN_E_UNSUPPORTED;
    if (workspace_bytes < nchw_layout(nchw_geom(d), nullptr).bytes) return CNSN_E_WORKSPACE;
    return nchw_backward(d, grad_y, x, addend, saved, grad_x, grad_addend, d_weight, d_bias, workspace, (hipStream_t)stream);
}

}  // extern "C"
