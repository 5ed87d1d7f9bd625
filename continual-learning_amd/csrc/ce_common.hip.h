// Pieces shared by the per-pixel loss kernels of misc.hip (ce4_kernel, ce4u_kernel) and pseudo.hip (ce4w_kernel): the partial-row count of
// the valid pixels, the one- or four-pixel accessors, and the store of the second, NHWC copy of d logits.
#pragma once
#include "common.hip.h"

namespace clamd {

// workgroups of count_valid_rows_kernel (clamd_ce_count): one partial {valid, bad} pair each
constexpr int CE_COUNT_BLOCKS = 256;
// total of column `col` of those rows, by every thread of a 256-thread workgroup (through `tmp`, 4 words of LDS)
__device__ inline unsigned int ce_count_total(const unsigned int* __restrict__ rows, int col, unsigned int* tmp) {
    static_assert(CE_COUNT_BLOCKS == 256, "one row per thread");
    unsigned int v = rows[2 * threadIdx.x + col];
    v += __shfl_xor(v, 32); v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    return tmp[0] + tmp[1] + tmp[2] + tmp[3];
}

struct ce_no_nhwc {};
#ifdef CE_NO_EXCHANGE      // A/B builds of the NHWC copy stored straight from the registers
#define CE_EXCHANGE false
#else
#define CE_EXCHANGE true
#endif
// The second copy of d logits of a lane's four consecutive pixels (v[k] = the gradient of class k), NHWC [pixel][dl_ldc] in dtype NT, channels
// K .. 31 zero: ce4_kernel's store block as a function, for ce4u_kernel (ce4_kernel keeps its inline copy: calling this there changed
// the register allocation of its NHWC instantiations).  XCH (bf16): through LDS, with two workgroup barriers -- every lane of the workgroup calls.
template <int KMAX, typename NT, bool XCH>
__device__ inline void ce_store_nhwc4(const float4 (&v)[KMAX], int K, NT* dl_nhwc, int dl_ldc, long long pix, long long base, long long nq,
                                      uint4 (*xbuf)[XCH ? 1024 : 1]) {
    if constexpr (XCH) {
        // A lane owns 4 pixels x 64 bytes; stored straight from its registers every instruction would write 16 bytes every 256 (64 partial
        // lines).  Instead the wave's 1024 16-byte pieces go through LDS (piece P = 16 lane + 4 q + cg at slot P ^ (lane & 7): the eight
        // lanes a ds_write_b128 is served in hit eight different bank groups; the reader undoes it with (P >> 4) & 7) and leave in pixel
        // order: one store instruction = 16 pixels x 64 bytes = 1 KB of contiguous output.
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {
                unsigned w[4];
#pragma unroll
                for (int j2 = 0; j2 < 4; ++j2) {
                    float e[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int k = cg * 8 + 2 * j2 + u;
                        float t = 0.f;
                        if (k < KMAX) { if (k < K) t = q == 0 ? v[k < KMAX ? k : 0].x : q == 1 ? v[k < KMAX ? k : 0].y : q == 2 ? v[k < KMAX ? k : 0].z : v[k < KMAX ? k : 0].w; }
                        e[u] = t;
                    }
                    w[j2] = (unsigned)f2bf(e[0]) | ((unsigned)f2bf(e[1]) << 16);
                }
                const int P = 16 * lane + 4 * q + cg;
                xbuf[wv][P ^ (lane & 7)] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        __syncthreads();
        const long long wave_pix = 4 * (base + 64 * wv);          // first pixel of this wave's 256
        const long long npix = 4 * nq;
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int P = 64 * it + lane;
            const long long px = wave_pix + (P >> 2);
            if (px < npix) *reinterpret_cast<uint4*>((uint16_t*)dl_nhwc + px * dl_ldc + (P & 3) * 8) = xbuf[wv][P ^ ((P >> 4) & 7)];
        }
        __syncthreads();
    } else if constexpr (!__is_same(NT, ce_no_nhwc)) {
        NT* o = dl_nhwc + pix * dl_ldc;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {          // 32 physical channels: four groups of eight
                float t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = cg * 8 + j;
                    float e = 0.f;
                    if (k < KMAX) { if (k < K) e = q == 0 ? v[k < KMAX ? k : 0].x : q == 1 ? v[k < KMAX ? k : 0].y : q == 2 ? v[k < KMAX ? k : 0].z : v[k < KMAX ? k : 0].w; }
                    t[j] = e;
                }
                Vec8<NT>::store(o + (long long)q * dl_ldc + cg * 8, t);
            }
    }
}

// NPX = 4: a lane's four consecutive pixels in the four components; NPX = 1: one pixel in .x
template <int NPX> __device__ inline float4 ce_ldpx(const float* p) {
    if constexpr (NPX == 4) return *reinterpret_cast<const float4*>(p);
    else return make_float4(*p, 0.f, 0.f, 0.f);
}
__device__ inline float& ce_at(float4& a, int c) { return c == 0 ? a.x : c == 1 ? a.y : c == 2 ? a.z : a.w; }
__device__ inline float ce_at(const float4& a, int c) { return c == 0 ? a.x : c == 1 ? a.y : c == 2 ? a.z : a.w; }

}  // namespace clamd
