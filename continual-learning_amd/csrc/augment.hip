// Training augmentation (build-defined, parity unpinned: the reference stops at Pad + CenterCrop + Normalize; include/clamd.h states the
// definition).
//   clamd_augment_batch        random scale, crop / pad and horizontal flip of an image batch and its label batch, one launch
// Per image a Q16 source pitch `step` and a Q16 origin (y0, x0): output pixel (i, j) samples the source at (y0 + i * step, x0 + j * step),
// all in 64-bit integers, so which label is taken and which pixels are padding never depends on floating-point rounding.  The image is
// bilinear (two horizontal lerps and a vertical one in fp32, weights = the low 16 bits of the coordinate), the label the nearest pixel.
// With W % 4 == 0 and aligned output bases a lane owns four consecutive output pixels of a row: the row's (rows, weight, inside) and the four
// pixels' (columns, weight, inside) are formed once and serve every channel; one 16-byte store per channel, two 16-byte label stores.  The
// taps are 4-byte gathers (their addresses depend on the params); neighbouring lanes read neighbouring taps, so the lines are shared in L1 /
// L2.  Any other width or alignment takes the one-pixel instantiation of the same arithmetic inside the same entry point.  Grid-stride with
// a capped grid; the only atomic is the guard's integer add.
#include <stdio.h>
#include "common.hip.h"
#include "clamd_internal.h"

namespace clamd {

constexpr long long AUG_STEP_MIN = 1ll << 13, AUG_STEP_MAX = 1ll << 19;      // scale 8 ... 1/8
constexpr int AUG_MAX_SIZE = 4096;
constexpr int AUG_GRID_CAP = 2048;       // 2048 workgroups of 4 waves: 8 waves on every SIMD of 256 CUs

struct alignas(16) aug_ll2 { long long a, b; };

// One axis of one output pixel: the two bilinear taps i0 / i1 (clamped), the weight of i1, the nearest pixel il, and whether the sample lies
// inside the source.  The sums wrap (unsigned) instead of overflowing for an origin near the ends of int64: a true coordinate outside
// [-2^63, 2^63) can only wrap to another value outside the source (idx * step <= 2^31).
struct aug_axis { int i0, i1, il; float w; bool in; };
__device__ inline aug_axis aug_coord(long long origin, long long step, int idx, int N) {
    const long long s = (long long)((unsigned long long)origin + (unsigned long long)idx * (unsigned long long)step);
    const long long t = (long long)((unsigned long long)s + 32768ull);
    aug_axis a;
    a.in = t >= 0 && t < ((long long)N << 16);
    a.il = a.in ? (int)(t >> 16) : 0;
    const long long f = s >> 16;
    a.i0 = (int)(f < 0 ? 0 : (f > N - 1 ? N - 1 : f));
    a.i1 = (int)(f + 1 < 0 ? 0 : (f + 1 > N - 1 ? N - 1 : f + 1));
    a.w = (float)(int)(s & 65535) * (1.f / 65536.f);
    return a;
}

// params[b] = {step, y0, x0, flags}.  A step outside [2^13, 2^19] gives an all-fill image and all-ignore labels and is counted once in bad.
// images / out_images or labels / out_labels may be NULL (as a pair).
template <int NPX>
__global__ void __launch_bounds__(256) augment_kernel(const float* __restrict__ images, const long long* __restrict__ labels,
                                                      const long long* __restrict__ params, int B, int C, int H, int W,
                                                      float* __restrict__ out_images, long long* __restrict__ out_labels, float fill,
                                                      long long ignore_index, unsigned int* bad) {
    const int Wg = W / NPX;                                  // groups per row
    const long long HW = (long long)H * W, per = (long long)H * Wg, total = (long long)B * per;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long b = i / per, q = i - b * per;
        const int y = (int)(q / Wg), xg = (int)(q - (long long)y * Wg);
        const long long p = (long long)y * W + (long long)NPX * xg;          // first pixel of the group in the output image
        const long long* pr = params + 4 * b;
        const long long step = pr[0], y0 = pr[1], x0 = pr[2];
        const bool flip = pr[3] & 1;
        const bool ok = step >= AUG_STEP_MIN && step <= AUG_STEP_MAX;
        if (!ok && q == 0) atomicAdd(bad, 1u);
        const aug_axis ay = aug_coord(y0, step, y, H);
        int c0[NPX], c1[NPX], cl[NPX];
        float wx[NPX];
        bool in[NPX];
#pragma unroll
        for (int k = 0; k < NPX; ++k) {
            const int jo = NPX * xg + k;
            const aug_axis ax = aug_coord(x0, step, flip ? W - 1 - jo : jo, W);
            c0[k] = ax.i0; c1[k] = ax.i1; cl[k] = ax.il; wx[k] = ax.w;
            in[k] = ok && ay.in && ax.in;
        }
        if (out_labels) {
            const long long* lb = labels + b * HW + (long long)ay.il * W;
            long long* ol = out_labels + b * HW + p;
            long long v[NPX];
#pragma unroll
            for (int k = 0; k < NPX; ++k) v[k] = in[k] ? lb[cl[k]] : ignore_index;
            if constexpr (NPX == 4) {
                const aug_ll2 u = {v[0], v[1]}, w = {v[2], v[3]};
                *reinterpret_cast<aug_ll2*>(ol) = u;
                *reinterpret_cast<aug_ll2*>(ol + 2) = w;
            } else *ol = v[0];
        }
        if (out_images) {
            const float* im = images + b * C * HW;
            float* oi = out_images + b * C * HW + p;
            const long long r0 = (long long)ay.i0 * W, r1 = (long long)ay.i1 * W;
            const float wy = ay.w;
            for (int c = 0; c < C; ++c) {
                const float* s0 = im + c * HW + r0;
                const float* s1 = im + c * HW + r1;
                float v[NPX];
#pragma unroll
                for (int k = 0; k < NPX; ++k) {
                    v[k] = fill;
                    if (in[k]) {
                        const float ta = s0[c0[k]], tb = s0[c1[k]], tc = s1[c0[k]], td = s1[c1[k]];
                        const float top = ta + wx[k] * (tb - ta), bot = tc + wx[k] * (td - tc);
                        v[k] = top + wy * (bot - top);
                    }
                }
                if constexpr (NPX == 4) *reinterpret_cast<float4*>(oi + c * HW) = make_float4(v[0], v[1], v[2], v[3]);
                else oi[c * HW] = v[0];
            }
        }
    }
}

}  // namespace clamd

using namespace clamd;

static inline bool al(const void* p, size_t a) { return ((size_t)p % a) == 0; }

extern "C" {

int clamd_augment_batch(const float* images, const long long* labels, const long long* params, int B, int C, int H, int W,
                        float* out_images, long long* out_labels, double fill, long long ignore_index, unsigned int* bad, void* stream) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return clamd_fail("augment_batch: empty problem");
    if (H > AUG_MAX_SIZE || W > AUG_MAX_SIZE) return clamd_fail("augment_batch: H and W must be at most 4096");
    if (!images != !out_images || !labels != !out_labels)
        return clamd_fail("augment_batch: images and out_images go together, and so do labels and out_labels");
    if (!images && !labels) return clamd_fail("augment_batch: neither images nor labels");
    if (!params || !bad) return clamd_fail("augment_batch: null params or bad");
    if (!al(images, 4) || !al(out_images, 4) || !al(labels, 8) || !al(out_labels, 8) || !al(params, 8) || !al(bad, 4))
        return clamd_fail("augment_batch: misaligned tensor");
    const bool four = W % 4 == 0 && al(out_images, 16) && al(out_labels, 32);
    const long long items = (long long)B * H * (W / (four ? 4 : 1)), blocks = (items + 255) / 256;
    const int g = (int)(blocks > AUG_GRID_CAP ? AUG_GRID_CAP : blocks);
    hipStream_t s = (hipStream_t)stream;
    if (four)
        hipLaunchKernelGGL(augment_kernel<4>, dim3(g), dim3(256), 0, s, images, labels, params, B, C, H, W, out_images, out_labels, (float)fill,
                           ignore_index, bad);
    else
        hipLaunchKernelGGL(augment_kernel<1>, dim3(g), dim3(256), 0, s, images, labels, params, B, C, H, W, out_images, out_labels, (float)fill,
                           ignore_index, bad);
    return clamd_check_launch("augment_batch");
}

}  // extern "C"
