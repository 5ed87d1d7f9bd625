// Pieces shared by the per-pixel kernels of loss.hip and pseudo.hip: the one- or four-pixel accessors, the label loader, the workgroup's partial
// pair and the finalize kernels' fp64 tree.
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

// the counterpart of ce_ldpx: g's four components, or .x
template <int NPX> __device__ inline void ce_stpx(float* p, const float4& g) {
    if constexpr (NPX == 4) *reinterpret_cast<float4*>(p) = g;
    else *p = g.x;
}

// A 256-thread workgroup's partial pair from the wave totals a (and b; !TWO: the second column is 0): the four waves added in order, by
// every thread of the workgroup (a barrier inside).
template <bool TWO> __device__ inline void ce_block_pair(float a, float b, float* __restrict__ partial) {
    __shared__ float red[TWO ? 2 : 1][4];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        if constexpr (TWO) red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x + 0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        if constexpr (TWO) partial[2 * blockIdx.x + 1] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        else partial[2 * blockIdx.x + 1] = 0.f;
    }
}

// The 256 threads' (a, b) added in fp64 in a fixed tree, by every thread of the workgroup -> the LDS rows; [c][0] holds column c's total.
using ce_tree_row = double[256];
__device__ inline const ce_tree_row* ce_tree_pair(double a, double b) {
    __shared__ double red[2][256];
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { red[0][threadIdx.x] += red[0][threadIdx.x + s]; red[1][threadIdx.x] += red[1][threadIdx.x + s]; }
        __syncthreads();
    }
    return red;
}

}  // namespace clamd
