// Phase B of the channels-last single-launch kernels (SelfNorm block: cnsn_nhwc_fused_kernels.h; bn3 in front of it:
// cnsn_nhwc_bnhead_kernels.h; IBN: cnsn_nhwc_ibn_kernels.h; BatchNorm2d + ReLU: cnsn_nhwc_bn_kernels.h): what the scalar
// algebra between the two grid barriers shares.  A workgroup takes GC adjacent channels, thread n holds the planes of instance
// n, and the threads j < GC own channel c0 + j.  Nothing here walks the tensor.
#pragma once
#include "cnsn_algebra.h"

namespace cnsn {

// the lane's value of a per-channel array in phase B: thread j < GC owns channel c0 + j
template <int GC>
__device__ __forceinline__ double pick(const double (&v)[GC], int j) {
    double r = 0.0;
#pragma unroll
    for (int q = 0; q < GC; ++q)
        if (q == j) r = v[q];
    return r;
}

// A BatchNorm's running buffers after a training step, by the lane that owns entry c: `var` is the BIASED batch variance (what
// normalises), the unbiased one goes to running_var (torch); momentum as given; the owner of entry 0 counts the step
__device__ __forceinline__ void running_update(float* run_mean, float* run_var, long long* nbt, int c, double mean, double var,
                                               double unbias, double mom) {
    run_mean[c] = (float)((1.0 - mom) * (double)run_mean[c] + mom * mean);
    run_var[c] = (float)((1.0 - mom) * (double)run_var[c] + mom * var * unbias);
    if (c == 0) bump_batches_tracked(nbt);
}

}  // namespace cnsn
