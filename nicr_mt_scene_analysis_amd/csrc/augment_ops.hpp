// augment_ops.hpp — what the two batch-augmentation kernels (augment.hip, augment_resize.hip) do to
// a source element once they have fetched it: stated once, so that a batch that is resized and one
// that is not normalise with the same instructions.
#pragma once
#include "nmsa_common.hpp"

namespace nmsa {

struct op_move {
    template <typename T>
    __device__ __forceinline__ T operator()(T v, int) const { return v; }
};

// one IEEE subtract, then one IEEE divide (the files are built with -ffp-contract=off)
struct op_rgb_norm {
    float mean[3], std[3];
    __device__ __forceinline__ float operator()(uint8_t v, int c) const { return ((float)v - mean[c]) / std[c]; }
};

struct op_depth_norm {
    float mean, std, invalid;
    bool raw;
    template <typename T>
    __device__ __forceinline__ float operator()(T v, int) const
    {
        const float f = (float)v;
        // the test is on the source value: -0.0 == 0.0 comes out as the invalid value itself (+0.0)
        return (raw && f == invalid) ? invalid : (f - mean) / std;
    }
};

}  // namespace nmsa
