// Pieces shared by the per-pixel kernels of loss.hip and pseudo.hip: the one- or four-pixel accessors and the label loader.
#pragma once
#include "common.hip.h"

namespace clamd {

// over the pixels of a thread
#define CE_PX _Pragma("unroll") for (int c = 0; c < NPX; ++c)

// NPX = 4: a lane's four consecutive pixels in the four components; NPX = 1: one pixel in .x
template <int NPX> __device__ inline float4 ce_ldpx(const float* p) {
    if constexpr (NPX == 4) return *reinterpret_cast<const float4*>(p);
    else return make_float4(*p, 0.f, 0.f, 0.f);
}
__device__ inline float& ce_at(float4& a, int c) { return c == 0 ? a.x : c == 1 ? a.y : c == 2 ? a.z : a.w; }
__device__ inline float ce_at(const float4& a, int c) { return c == 0 ? a.x : c == 1 ? a.y : c == 2 ? a.z : a.w; }

template <int NPX> __device__ inline void ce_ld_labels(const long long* __restrict__ labels, long long pix, long long (&lab)[4]) {
    if constexpr (NPX == 4) *reinterpret_cast<longlong4*>(lab) = *reinterpret_cast<const longlong4*>(labels + pix);
    else lab[0] = labels[pix];
}

}  // namespace clamd
