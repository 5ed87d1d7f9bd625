// Exemplar replay (build-defined, parity unpinned: the reference has no continual-learning code; rehearsal as include/clamd.h restates it).
//   clamd_class_pixel_counts   per-image class histogram of a label batch: what the class-balanced fill policy reads (once per task)
//   clamd_replay_store         n images of a batch into slots of the on-device store (uint8 or fp32 images, uint8 labels), one launch
//   clamd_replay_mix           the training batch of a step: the B current images bit-copied, R exemplars decoded and flipped, one launch
// The two copy kernels are HBM-bound byte movers.  With W % 4 == 0 and aligned bases a lane handles four consecutive pixels of a row: one
// 4-byte access per uint8 channel, one 16-byte access per fp32 channel, two 16-byte accesses for the int64 labels; a horizontal flip reverses
// the four pixels inside the lane and mirrors the group index along the row.  Any other width or alignment takes the one-pixel variant of the
// same arithmetic inside the same entry point.  Grid-stride with a capped grid throughout; integer atomics only.
#include <stdio.h>
#include "common.hip.h"
#include "clamd_internal.h"

namespace clamd {

// what the store holds for a label: itself in [0, K), 255 for ignore_index and for anything else (the latter counted by the caller)
__device__ inline unsigned int replay_enc_label(long long l, int K, long long ignore_index, unsigned int& nbad) {
    if (l == ignore_index) return 255u;
    if (l >= 0 && l < K) return (unsigned int)l;
    ++nbad;
    return 255u;
}
__device__ inline long long replay_dec_label(unsigned int u, long long ignore_index) { return u == 255u ? ignore_index : (long long)u; }

// x in [-1, 1] -> byte, in fp32: the inverse of Normalize(0.5, 0.5) after ToTensor, rounded to nearest even, clamped.  A NaN gives 0.
__device__ inline unsigned int replay_enc_px(float x) {
    const float t = rintf((x * 0.5f + 0.5f) * 255.f);
    return (unsigned int)(int)fminf(fmaxf(t, 0.f), 255.f);
}
// byte -> x: voc_prepare_kernel's arithmetic (misc.hip), ToTensor then Normalize(0.5, 0.5)
__device__ inline float replay_dec_px(unsigned int u) {
    const float v = (float)u / 255.f;
    return (v - 0.5f) / 0.5f;
}
__device__ inline unsigned int replay_rev4(unsigned int w) { return __builtin_bswap32(w); }

struct alignas(16) ll2 { long long a, b; };

// counts[b][k] += pixels of image b with label k.  A workgroup takes (image, chunk of CHUNK pixels) jobs: a histogram in LDS (integer
// atomics), added to the image's row with one integer atomic per non-empty class.  NPX = 4: 32-byte label loads.
constexpr int COUNT_CHUNK = 2048;
template <int NPX>
__global__ void __launch_bounds__(256) class_counts_kernel(const long long* __restrict__ labels, int* counts, unsigned int* bad, int B, int K,
                                                           long long HW, int nchunk, long long ignore_index) {
    __shared__ unsigned int lh[256];
    unsigned int nbad = 0;
    const long long njobs = (long long)B * nchunk;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) {
        const long long b = job / nchunk, p0 = (job - b * nchunk) * COUNT_CHUNK;
        const long long p1 = p0 + COUNT_CHUNK < HW ? p0 + COUNT_CHUNK : HW;
        lh[threadIdx.x] = 0;
        __syncthreads();
        const long long* row = labels + b * HW;
        for (long long p = p0 + NPX * (long long)threadIdx.x; p < p1; p += NPX * 256) {      // HW % NPX == 0: a group never crosses p1
            long long lab[NPX];
            if constexpr (NPX == 4) {
                const ll2 u = *reinterpret_cast<const ll2*>(row + p), v = *reinterpret_cast<const ll2*>(row + p + 2);
                lab[0] = u.a; lab[1] = u.b; lab[2] = v.a; lab[3] = v.b;
            } else lab[0] = row[p];
#pragma unroll
            for (int c = 0; c < NPX; ++c) {
                const long long l = lab[c];
                if (l == ignore_index) continue;
                if (l >= 0 && l < K) atomicAdd(&lh[(int)l], 1u);
                else ++nbad;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < K && lh[threadIdx.x]) atomicAdd(&counts[b * K + threadIdx.x], (int)lh[threadIdx.x]);
        __syncthreads();
    }
    if (nbad) atomicAdd(bad, nbad);
}

// store[slot[r]] = encode(batch[src[r]]) for r < n.  An index outside the batch or the store (the host policy never produces one) moves
// nothing and is counted in bad by the row's first item.
template <bool FP32, int NPX>
__global__ void __launch_bounds__(256) replay_store_kernel(const float* __restrict__ images, const long long* __restrict__ labels,
                                                           const int* __restrict__ src, const int* __restrict__ slot, int n,
                                                           void* store_images, unsigned char* store_labels, int cap, unsigned int* bad,
                                                           int B, int C, long long HW, int K, long long ignore_index) {
    const long long per = HW / NPX, total = (long long)n * per;
    unsigned int nbad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / per, p = NPX * (i - r * per);
        const int s = src[r], d = slot[r];
        if (s < 0 || s >= B || d < 0 || d >= cap) {
            if (p == 0) ++nbad;
            continue;
        }
        const float* im = images + (long long)s * C * HW + p;
        const long long* lb = labels + (long long)s * HW + p;
        unsigned char* dl = store_labels + (long long)d * HW + p;
        if constexpr (NPX == 4) {
            for (int c = 0; c < C; ++c) {
                const float4 x = *reinterpret_cast<const float4*>(im + c * HW);
                if constexpr (FP32) *reinterpret_cast<float4*>((float*)store_images + ((long long)d * C + c) * HW + p) = x;
                else
                    *reinterpret_cast<unsigned int*>((unsigned char*)store_images + ((long long)d * C + c) * HW + p) =
                        replay_enc_px(x.x) | (replay_enc_px(x.y) << 8) | (replay_enc_px(x.z) << 16) | (replay_enc_px(x.w) << 24);
            }
            const ll2 u = *reinterpret_cast<const ll2*>(lb), v = *reinterpret_cast<const ll2*>(lb + 2);
            *reinterpret_cast<unsigned int*>(dl) = replay_enc_label(u.a, K, ignore_index, nbad) | (replay_enc_label(u.b, K, ignore_index, nbad) << 8) |
                                                   (replay_enc_label(v.a, K, ignore_index, nbad) << 16) | (replay_enc_label(v.b, K, ignore_index, nbad) << 24);
        } else {
            for (int c = 0; c < C; ++c) {
                const float x = im[c * HW];
                if constexpr (FP32) ((float*)store_images)[((long long)d * C + c) * HW + p] = x;
                else ((unsigned char*)store_images)[((long long)d * C + c) * HW + p] = (unsigned char)replay_enc_px(x);
            }
            *dl = (unsigned char)replay_enc_label(*lb, K, ignore_index, nbad);
        }
    }
    if (nbad) atomicAdd(bad, nbad);
}

// out rows [0, B) = the current batch, bit for bit; out rows [B, B + R) = exemplar slots[r] decoded, flipped by flips[r] (bit 0: along W,
// bit 1: along H; NULL: none).  A slot outside [0, cap) gives a zero image and all-ignore labels and is counted once in bad.
template <bool FP32, int NPX>
__global__ void __launch_bounds__(256) replay_mix_kernel(const float* __restrict__ cur_images, const long long* __restrict__ cur_labels, int B,
                                                         const void* __restrict__ store_images, const unsigned char* __restrict__ store_labels,
                                                         int cap, const long long* __restrict__ slots, const int* __restrict__ flips, int R,
                                                         float* __restrict__ out_images, long long* __restrict__ out_labels, unsigned int* bad,
                                                         int C, int H, int W, long long ignore_index) {
    const int Wg = W / NPX;                                  // groups per row
    const long long HW = (long long)H * W, per = (long long)H * Wg, total = (long long)(B + R) * per;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long row = i / per, q = i - row * per;
        const int y = (int)(q / Wg), xg = (int)(q - (long long)y * Wg);
        const long long p = (long long)y * W + (long long)NPX * xg;          // first pixel of the group in the output image
        float* oi = out_images + row * C * HW + p;
        long long* ol = out_labels + row * HW + p;
        if (row < B) {
            const float* im = cur_images + row * C * HW + p;
            const long long* lb = cur_labels + row * HW + p;
            if constexpr (NPX == 4) {
                for (int c = 0; c < C; ++c) *reinterpret_cast<float4*>(oi + c * HW) = *reinterpret_cast<const float4*>(im + c * HW);
                *reinterpret_cast<ll2*>(ol) = *reinterpret_cast<const ll2*>(lb);
                *reinterpret_cast<ll2*>(ol + 2) = *reinterpret_cast<const ll2*>(lb + 2);
            } else {
                for (int c = 0; c < C; ++c) oi[c * HW] = im[c * HW];
                *ol = *lb;
            }
            continue;
        }
        const int r = (int)(row - B);
        const long long s = slots[r];
        if (s < 0 || s >= cap) {
            if (q == 0) atomicAdd(bad, 1u);
            if constexpr (NPX == 4) {
                for (int c = 0; c < C; ++c) *reinterpret_cast<float4*>(oi + c * HW) = make_float4(0.f, 0.f, 0.f, 0.f);
                const ll2 ig = {ignore_index, ignore_index};
                *reinterpret_cast<ll2*>(ol) = ig;
                *reinterpret_cast<ll2*>(ol + 2) = ig;
            } else {
                for (int c = 0; c < C; ++c) oi[c * HW] = 0.f;
                *ol = ignore_index;
            }
            continue;
        }
        const int f = flips ? flips[r] : 0;
        const bool fw = f & 1;
        const int sy = (f & 2) ? H - 1 - y : y, sxg = fw ? Wg - 1 - xg : xg;
        const long long sp = (long long)sy * W + (long long)NPX * sxg;        // first pixel of the source group in the stored image
        const unsigned char* sl = store_labels + s * HW + sp;
        if constexpr (NPX == 4) {
            for (int c = 0; c < C; ++c) {
                float4 x;
                if constexpr (FP32) {
                    x = *reinterpret_cast<const float4*>((const float*)store_images + (s * C + c) * HW + sp);
                    if (fw) x = make_float4(x.w, x.z, x.y, x.x);
                } else {
                    unsigned int w = *reinterpret_cast<const unsigned int*>((const unsigned char*)store_images + (s * C + c) * HW + sp);
                    if (fw) w = replay_rev4(w);
                    x = make_float4(replay_dec_px(w & 255u), replay_dec_px((w >> 8) & 255u), replay_dec_px((w >> 16) & 255u), replay_dec_px(w >> 24));
                }
                *reinterpret_cast<float4*>(oi + c * HW) = x;
            }
            unsigned int w = *reinterpret_cast<const unsigned int*>(sl);
            if (fw) w = replay_rev4(w);
            const ll2 u = {replay_dec_label(w & 255u, ignore_index), replay_dec_label((w >> 8) & 255u, ignore_index)};
            const ll2 v = {replay_dec_label((w >> 16) & 255u, ignore_index), replay_dec_label(w >> 24, ignore_index)};
            *reinterpret_cast<ll2*>(ol) = u;
            *reinterpret_cast<ll2*>(ol + 2) = v;
        } else {
            for (int c = 0; c < C; ++c) {
                if constexpr (FP32) oi[c * HW] = ((const float*)store_images)[(s * C + c) * HW + sp];
                else oi[c * HW] = replay_dec_px(((const unsigned char*)store_images)[(s * C + c) * HW + sp]);
            }
            *ol = replay_dec_label(*sl, ignore_index);
        }
    }
}

}  // namespace clamd

using namespace clamd;

static int replay_grid(long long items, int cap) {
    long long g = (items + 255) / 256;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}
static inline bool al(const void* p, size_t a) { return ((size_t)p % a) == 0; }

extern "C" {

int clamd_class_pixel_counts(const long long* labels, int* counts, unsigned int* bad, int B, int K, int H, int W, long long ignore_index,
                             void* stream) {
    if (!labels || !counts || !bad) return clamd_fail("class_pixel_counts: null labels, counts or bad");
    if (B <= 0 || H <= 0 || W <= 0) return clamd_fail("class_pixel_counts: empty shape");
    if (K < 1 || K > 255) return clamd_fail("class_pixel_counts: K must be in [1, 255] (the workgroup's histogram has 256 LDS words)");
    if (!al(labels, 8) || !al(counts, 4) || !al(bad, 4)) return clamd_fail("class_pixel_counts: misaligned tensor");
    const long long HW = (long long)H * W;
    const int nchunk = (int)((HW + COUNT_CHUNK - 1) / COUNT_CHUNK);
    if ((long long)B * nchunk > 0x7fffffffLL || (long long)B * K > 0x7fffffffLL) return clamd_fail("class_pixel_counts: batch too large");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * K * sizeof(int), s) != hipSuccess) return clamd_fail("class_pixel_counts: memset failed");
    const long long njobs = (long long)B * nchunk;
    const int g = (int)(njobs > 2048 ? 2048 : njobs);
    if (HW % 4 == 0 && al(labels, 32))
        hipLaunchKernelGGL(class_counts_kernel<4>, dim3(g), dim3(256), 0, s, labels, counts, bad, B, K, HW, nchunk, ignore_index);
    else
        hipLaunchKernelGGL(class_counts_kernel<1>, dim3(g), dim3(256), 0, s, labels, counts, bad, B, K, HW, nchunk, ignore_index);
    return clamd_check_launch("class_pixel_counts");
}

int clamd_replay_store(const float* images, const long long* labels, const int* src, const int* slot, int n, void* store_images,
                       unsigned char* store_labels, int store_fp32, int cap, unsigned int* bad, int B, int C, int H, int W, int K,
                       long long ignore_index, void* stream) {
    if (!images || !labels || !src || !slot || !store_images || !store_labels || !bad) return clamd_fail("replay_store: null pointer");
    if (n <= 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || cap <= 0) return clamd_fail("replay_store: empty shape, batch or store");
    if (n > cap) return clamd_fail("replay_store: more images than slots (the slots of one call must be distinct)");
    if (K < 1 || K > 255) return clamd_fail("replay_store: K must be in [1, 255] (255 is the stored ignore value)");
    if (store_fp32 != 0 && store_fp32 != 1) return clamd_fail("replay_store: store_fp32 must be 0 or 1");
    if (!al(images, 4) || !al(labels, 8) || !al(src, 4) || !al(slot, 4) || !al(bad, 4) || (store_fp32 && !al(store_images, 4)))
        return clamd_fail("replay_store: misaligned tensor");
    const long long HW = (long long)H * W;
    const bool four = W % 4 == 0 && al(images, 16) && al(labels, 32) && al(store_images, store_fp32 ? 16 : 4) && al(store_labels, 4);
    const int g = replay_grid((long long)n * (HW / (four ? 4 : 1)), 2048);
    hipStream_t s = (hipStream_t)stream;
#define RS(F_, N_) hipLaunchKernelGGL((replay_store_kernel<F_, N_>), dim3(g), dim3(256), 0, s, images, labels, src, slot, n, store_images, store_labels, cap, bad, B, C, HW, K, ignore_index)
    if (store_fp32) { if (four) RS(true, 4); else RS(true, 1); }
    else { if (four) RS(false, 4); else RS(false, 1); }
#undef RS
    return clamd_check_launch("replay_store");
}

int clamd_replay_mix(const float* cur_images, const long long* cur_labels, int B, const void* store_images, const unsigned char* store_labels,
                     int store_fp32, int cap, const long long* slots, const int* flips, int R, float* out_images, long long* out_labels,
                     unsigned int* bad, int C, int H, int W, long long ignore_index, void* stream) {
    if (B < 0 || R < 0 || B + (long long)R <= 0 || B + (long long)R > 0x7fffffffLL) return clamd_fail("replay_mix: B and R must be >= 0 and not both 0");
    if (C <= 0 || H <= 0 || W <= 0) return clamd_fail("replay_mix: empty shape");
    if (B > 0 && (!cur_images || !cur_labels)) return clamd_fail("replay_mix: B > 0 needs the current images and labels");
    if (R > 0 && (!store_images || !store_labels || !slots || cap <= 0)) return clamd_fail("replay_mix: R > 0 needs the store and the slots");
    if (!out_images || !out_labels || !bad) return clamd_fail("replay_mix: null out_images, out_labels or bad");
    if (store_fp32 != 0 && store_fp32 != 1) return clamd_fail("replay_mix: store_fp32 must be 0 or 1");
    if (!al(cur_images, 4) || !al(cur_labels, 8) || !al(out_images, 4) || !al(out_labels, 8) || !al(slots, 8) || !al(flips, 4) || !al(bad, 4) ||
        (store_fp32 && !al(store_images, 4)))
        return clamd_fail("replay_mix: misaligned tensor");
    const long long HW = (long long)H * W;
    const bool four = W % 4 == 0 && al(cur_images, 16) && al(cur_labels, 32) && al(out_images, 16) && al(out_labels, 32) &&
                      al(store_images, store_fp32 ? 16 : 4) && al(store_labels, 4);
    const int g = replay_grid((long long)(B + R) * (HW / (four ? 4 : 1)), 2048);
    hipStream_t s = (hipStream_t)stream;
#define RM(F_, N_) hipLaunchKernelGGL((replay_mix_kernel<F_, N_>), dim3(g), dim3(256), 0, s, cur_images, cur_labels, B, store_images, store_labels, cap, slots, flips, R, out_images, out_labels, bad, C, H, W, ignore_index)
    if (store_fp32) { if (four) RM(true, 4); else RM(true, 1); }
    else { if (four) RM(false, 4); else RM(false, 1); }
#undef RM
    return clamd_check_launch("replay_mix");
}

}  // extern "C"
