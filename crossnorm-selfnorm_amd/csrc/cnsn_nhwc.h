// Channels-last two-pass path: host entry points (cnsn_nhwc.hip).  `cnsn_problem_t.layout` = CNSN_LAYOUT_NHWC.
#pragma once
#include <type_traits>

#include "cnsn_host_plan.h"

namespace cnsn {

// ---- pure host helpers of every channels-last unit (no kernels here: cnsn_nhwc.hip includes this header alone)
namespace nhwc_host {

inline int vec_of(int dtype) { return 16 / elem_bytes(dtype); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <typename F>
bool dispatch_t(int dtype, F&& f) {
    if (dtype == CNSN_F32) return f(TypeTag<float>{}, IntTag<4>{}), true;
    if (dtype == CNSN_BF16) return f(TypeTag<bf16_t>{}, IntTag<8>{}), true;
    if (dtype == CNSN_F16) return f(TypeTag<_Float16>{}, IntTag<8>{}), true;
    return false;
}

template <typename F>
void with_add(int add, F&& f) {  // (the kernels' AddMode has the C ABI's values)
    if (add == CNSN_ADD_PRE)
        f(IntTag<CNSN_ADD_PRE>{});
    else if (add == CNSN_ADD_POST)
        f(IntTag<CNSN_ADD_POST>{});
    else
        f(IntTag<CNSN_ADD_NONE>{});
}

template <typename F>
void with_flag(bool on, F&& f) {
    if (on)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// A caller-owned workspace handed out region by region, each starting on a 256-byte boundary.  On a null base it only counts, so
// ONE layout function per kernel family is both its size function and its launch path's pointers: the two cannot drift apart
// (the last region is the barrier block a persistent grid spins on).  bytes(): the regions + the 256 spare bytes the sizes include.
struct Carver {
    char* base;
    size_t used = 0;
    explicit Carver(void* workspace) : base((char*)workspace) {}
    template <typename T = float>
    T* take(size_t bytes) {
        T* p = base ? (T*)(base + used) : nullptr;
        used += align256(bytes);
        return p;
    }
    size_t bytes() const { return used + 256; }
};

// The first read of a single launch keeps the default cache policy when the second one can find it on chip (what phase A reads
// within reach of the 256 MiB Infinity Cache); non-temporal like every other single-use access beyond that.  `tensors`: how
// many tensors of `tensor_bytes` the launch has in flight between the two reads.
inline int keep_first_read(int tensors, size_t tensor_bytes) { return (size_t)tensors * tensor_bytes <= ((size_t)320 << 20) ? 1 : 0; }

}  // namespace nhwc_host

// the un-boxed op on a channels-last tensor whose channel count is a whole number of 16-byte vectors, no channel permutation
bool nhwc_supported(const Plan& pl, bool has_chan_perm);
// bytes the channels-last path needs behind the two-pass workspace (partial sums of the pixel chunks, plane-order rows)
size_t nhwc_extra_bytes(const Plan& pl);
// sum_out (ADD_PRE only, may be null, may alias x): where X = x + addend is kept (cnsn_epilogue_t.sum_out, ABI 8)
int nhwc_forward(Plan& pl, int add, int relu, const void* x, const void* addend, const int64_t* perm, GateDev g, GateDev f, void* y,
                 float* saved, void* workspace, size_t workspace_bytes, hipStream_t stream, void* sum_out = nullptr);
int nhwc_backward(Plan& pl, int add, int relu, const void* gy, const void* x, const void* addend, const int64_t* perm, GateDev g,
                  GateDev f, const float* saved, void* dx, void* d_addend, GateGradDev dg, GateGradDev df, void* workspace,
                  size_t workspace_bytes, hipStream_t stream);

// whole workspace a channels-last call may need (either strategy)
size_t nhwc_workspace_bytes(const Plan& pl);

// ---- single-launch kernels (cnsn_nhwc_fused.hip; SelfNorm alone, one gate, N <= 256) and the slim `saved` record they share with
// the two-pass kernels (cnsn_nhwc_fused_kernels.h)
bool nhwc_slim_record(const Plan& pl);  // this call's `saved` is the slim record (channels-last, no CrossNorm, one gate)
bool nhwc_fused_ok(const Plan& pl, bool check_health = true);  // the single-launch kernels take the call (strategy, switches, health, shape)
size_t nhwc_fused_extra_bytes(const Plan& pl);
int nhwc_fused_forward(Plan& pl, int add, int relu, const void* x, const void* addend, GateDev g, void* y, float* saved,
                       void* workspace, size_t workspace_bytes, hipStream_t stream, void* sum_out = nullptr);
int nhwc_fused_backward(Plan& pl, int add, int relu, const void* gy, const void* x, const void* addend, GateDev g,
                        const float* saved, void* dx, void* d_addend, GateGradDev dg, void* workspace, size_t workspace_bytes,
                        hipStream_t stream);
void nhwc_slim_from_saved(const Plan& pl, const double* saved_d, float* slim, hipStream_t stream);
void nhwc_saved_from_slim(const Plan& pl, const float* slim, int relu, double* saved_d, float* rows, hipStream_t stream);

// ---- the block's last BatchNorm2d in front of the op (cnsn_nhwc_bnhead_kernels.h; training mode, SelfNorm alone, one gate, N <= 256)
bool nhwc_bnhead_ok(const Plan& pl, bool check_health = true);
size_t nhwc_bnhead_extra_bytes(const Plan& pl);
// bn2 (may be null): the skip path ends in a BatchNorm2d of its own — `identity` is then ITS input (the downsample convolution's output).
// add: ADD_PRE as above; ADD_POST / ADD_NONE (pos='residual': act(SelfNorm(BatchNorm2d(conv_out)) [+ identity]); bn2 null, NONE without
// ReLU and without identity; the backward writes d_identity for POST with the ReLU only)
int nhwc_bnhead_forward(Plan& pl, int add, int relu, const cnsn_bn_tail_t& bn, const cnsn_bn_tail_t* bn2, const void* conv_out, const void* identity,
                        GateDev gg, void* y, float* saved, float* bn_stats, void* workspace, size_t workspace_bytes, hipStream_t stream);
int nhwc_bnhead_backward(Plan& pl, int add, int relu, const cnsn_bn_tail_t& bn, const cnsn_bn_tail_t* bn2, const void* gy, const void* conv_out,
                         const void* identity, GateDev gg, const float* saved, const float* bn_stats, void* d_conv, void* d_identity,
                         GateGradDev dg, float* dbn_w, float* dbn_b, float* dbn2_w, float* dbn2_b, void* workspace,
                         size_t workspace_bytes, hipStream_t stream);

}  // namespace cnsn
