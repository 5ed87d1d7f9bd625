// Remaining pieces of the train-step path: error plumbing, weight re-packing (fp32 NCHW-style master parameters ->
// the K-innermost compute-dtype layouts the implicit-GEMM kernels read) and the GPU-resident arg-max/confusion-matrix instrument
// (SURVEY.md §8f row 1).  The per-pixel loss is loss.hip, the optimisers are optim.hip.
#include <string.h>
#include <stdio.h>
#include "common.hip.h"
#include "clamd_internal.h"
#include "../../include/clamd_debug.h"

static thread_local char g_err[512] = "";

int clamd_fail(const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return -1;
}
int clamd_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -2;
}

int clamd_check_tuning(const clamd_tuning* t) {
    if (!t) return 0;
    if (t->igemm_pws < 0 || t->igemm_pws > 2) return clamd_fail("tuning: igemm_pws 0..2");
    if (t->igemm_ws < 0 || t->igemm_ws > 4) return clamd_fail("tuning: igemm_ws 0..4");
#ifndef CLAMD_DIAG
    if (t->igemm_variant < 0 || t->igemm_variant > 2) return clamd_fail("tuning: igemm_variant 0..2 (3..6 are timing ablations of the diagnostic build)");
#endif
    if (t->wgrad_dma < 0 || t->wgrad_dma > 2) return clamd_fail("tuning: wgrad_dma 0..2");
    if (t->wgrad_blocks < 1 || t->wgrad_blocks > 1024) return clamd_fail("tuning: wgrad_blocks 1..1024");
    if (t->wino_band < 0 || t->wino_band > 32) return clamd_fail("tuning: wino_band 0..32");
    if (t->wino_mt < 0 || t->wino_mt > 2) return clamd_fail("tuning: wino_mt 0..2");
    if (t->bn_reduce_blocks < 0 || t->bn_reduce_blocks > 65535) return clamd_fail("tuning: bn_reduce_blocks 0..65535");
    if (t->chsum_blocks < 0 || t->chsum_blocks > 1024) return clamd_fail("tuning: chsum_blocks 0..1024");
    if (t->cu_reserve < 0 || t->cu_reserve > 128) return clamd_fail("tuning: cu_reserve 0..128");
    if (t->wino_half < 0 || t->wino_half > 1) return clamd_fail("tuning: wino_half 0..1");
    if (t->wgrad_streamk < 0 || t->wgrad_streamk > 2) return clamd_fail("tuning: wgrad_streamk 0..2");
    return 0;
}

namespace clamd {

// ------------------------------------------------------------------------------------------------ pack
struct PackJob {
    const float* src;
    void* dst;
    int T, Np, Kp;               // physical extents iterated
    int N, K;                    // logical extents
    long long st, sn, sk;        // source strides (elements) of logical (t, n, k)
    long long dt, dn, dk;        // destination strides (elements) of physical (t, n, k)
    int n_seg0, n_seg0p;         // physical n -> logical: n < n_seg0p ? (n < n_seg0 ? n : pad) : n_seg0 + (n - n_seg0p)
    int k_seg0, k_seg0p;
    int flip;                    // read source tap T-1-t (spatially flipped filter for the data gradient)
    int dst_f32;                 // destination element type: 1 = float, 0 = compute dtype of the launch
    int block0;                  // first block of this job in the fused launch
    int kc;                      // 0: dst = t*dt + n*dn + k*dk;  >0: K-chunk-major  ((k/kc)*T + t)*Np*kc + n*kc + k%kc
                                 // (the 3x3 kernels read whole [tap][n] slabs of one K-chunk: contiguous 128-B lines)
    const float* kscale;         // optional [Kp]: every element is multiplied by kscale[physical k] (a BatchNorm folded into the
                                 // filters of the convolution behind it, bnfold.hip)
    void* dst_t;                 // optional second destination (kc > 0 only): the tap-flipped TRANSPOSED layout of the same tile, element
                                 // (T-1-t, n' = k, k' = n) K-chunk-major over n with the same kc -- the data-gradient filters of a 3x3
                                 // convolution from the one read of the source (kscale is NOT applied to it)
};

__device__ inline int phys2log(int p, int seg0, int seg0p, int L) {
    if (p < seg0p) return p < seg0 ? p : -1;
    const int l = seg0 + (p - seg0p);
    return l < L ? l : -1;
}

// One 256-thread block re-packs a 32(n) x 32(k) x T(taps <= 9) tile through LDS: the global reads run with lanes
// along whichever logical dimension is contiguous in the SOURCE (k for the forward layouts, n for the transposed
// data-gradient layouts), the global writes always with lanes along the destination's contiguous k -- both sides
// coalesced (the first version read with a 36-byte lane stride and fetched ~9x the bytes it needed).
constexpr int PACK_TILE = 32;
template <typename T>
__global__ void __launch_bounds__(256) pack_kernel(const PackJob* __restrict__ jobs, int njobs, int nblocks, const FoldBias fold) {
    __shared__ float tile[9][PACK_TILE][PACK_TILE + 1];
    if ((int)blockIdx.x >= nblocks) {       // appended blocks: the border-class bias table of a folded BatchNorm (common.hip.h)
        fold_bias_block(fold, (int)blockIdx.x - nblocks, &tile[0][0][0]);
        return;
    }
    int lo = 0, hi = njobs - 1;          // locate the job of this block (jobs are sorted by block0)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackJob j = jobs[lo];
    const int local = (int)blockIdx.x - j.block0;
    const int tiles_k = (j.Kp + PACK_TILE - 1) / PACK_TILE;
    const int n0 = (local / tiles_k) * PACK_TILE, k0 = (local % tiles_k) * PACK_TILE;
    const bool along_n = j.sn < j.sk;    // source-contiguous logical dimension gets the lanes
    const int tid = threadIdx.x;
#ifndef PACK_NO_RUN_PATH      // -DPACK_NO_RUN_PATH: A/B builds of the generic path alone
    if constexpr (!__is_same(T, float)) {
        // 3x3 filters into the K-chunk-major layouts (96 % of the bytes of a step's pack): [Cout][Cin][3][3] has 32 channels x 9 taps = 288
        // CONTIGUOUS floats per row of the tile -- rows = n for the forward layout (sk == 9), rows = k for the transposed data-gradient layout
        // (sn == 9) -- so the tile is read as whole 1152-byte runs (16-byte loads when the runs are aligned) and written as 16-byte pieces of
        // the destination's contiguous 2-KB (tap, 32 n) blocks.  The generic path below reads with a 36-byte lane stride and writes 2 bytes
        // per lane: 1.4 TB/s; the same bits.
        const bool rows_n = j.sk == 9, rows_k = j.sn == 9;
        constexpr int KCT = __is_same(T, bf16_t) ? 32 : 16;
        if (j.T == 9 && j.st == 1 && j.kc == KCT && !j.dst_f32 && rows_n != rows_k && j.Np % 8 == 0 && j.Kp % 8 == 0 && (!j.dst_t || rows_n)) {
            float (*tf)[289] = reinterpret_cast<float (*)[289]>(&tile[0][0][0]);      // 32 rows x 288 (+1) floats
            const int c0 = rows_n ? k0 : n0, r0 = rows_n ? n0 : k0;                     // contiguous / row dimension: first physical index
            const int cs0 = rows_n ? j.k_seg0 : j.n_seg0, cs0p = rows_n ? j.k_seg0p : j.n_seg0p, cL = rows_n ? j.K : j.N;
            const int rs0 = rows_n ? j.n_seg0 : j.k_seg0, rs0p = rows_n ? j.n_seg0p : j.k_seg0p, rL = rows_n ? j.N : j.K;
            // a 32-aligned tile never straddles the two segments (their physical sizes are multiples of 32): its logical channels are one run
            const int l0 = c0 < cs0p ? c0 : cs0 + (c0 - cs0p);
            const int lim = c0 < cs0p ? cs0 : cL;
            int nv = lim - l0;
            nv = nv < 0 ? 0 : (nv > PACK_TILE ? PACK_TILE : nv);
            const int run = nv * 9;
            const long long srow = rows_n ? j.sn : j.sk;
            const float* base = j.src + (long long)l0 * 9;
            const bool vec = nv == PACK_TILE && (srow & 3) == 0 && ((reinterpret_cast<uintptr_t>(base) & 15) == 0);
            if (vec) {
                for (int idx = tid; idx < PACK_TILE * 72; idx += 256) {
                    const int row = idx / 72, e4 = idx - row * 72;
                    const int lr = phys2log(r0 + row, rs0, rs0p, rL);
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (lr >= 0) v = *reinterpret_cast<const float4*>(base + lr * srow + 4 * e4);
                    tf[row][4 * e4] = v.x; tf[row][4 * e4 + 1] = v.y; tf[row][4 * e4 + 2] = v.z; tf[row][4 * e4 + 3] = v.w;
                }
            } else {
                for (int idx = tid; idx < PACK_TILE * 288; idx += 256) {
                    const int row = idx / 288, e = idx - row * 288;
                    const int lr = phys2log(r0 + row, rs0, rs0p, rL);
                    tf[row][e] = (lr >= 0 && e < run) ? base[lr * srow + e] : 0.f;
                }
            }
            __syncthreads();
            for (int item = tid; item < 9 * 128; item += 256) {
                const int t = item >> 7, nn = (item & 127) >> 2, k8 = item & 3;
                const int ts = j.flip ? 8 - t : t;
                const int n = n0 + nn, k = k0 + 8 * k8;
                if (n >= j.Np || k >= j.Kp) continue;
                float v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float x = rows_n ? tf[nn][(8 * k8 + i) * 9 + ts] : tf[8 * k8 + i][nn * 9 + ts];
                    // the scale of a padded channel is never read (the caller may leave it uninitialised): its filter entries are zeros
                    const bool kreal = rows_n ? 8 * k8 + i < nv : phys2log(k + i, rs0, rs0p, rL) >= 0;
                    v[i] = (j.kscale && kreal) ? x * j.kscale[k + i] : x;
                }
                const long long d = (((long long)(k / KCT) * 9 + t) * j.Np + n) * KCT + (k % KCT);      // element offset of (t, n, k)
                if constexpr (__is_same(T, bf16_t)) {
                    *reinterpret_cast<uint4*>((uint16_t*)j.dst + d) =
                        make_uint4((unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16), (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16),
                                   (unsigned)f2bf(v[4]) | ((unsigned)f2bf(v[5]) << 16), (unsigned)f2bf(v[6]) | ((unsigned)f2bf(v[7]) << 16));
                } else {
                    // 4 bytes per element: every 16-channel group is [16 x bf16 hi][16 x bf16 lo]; this item is 8 channels of one group
                    unsigned hi[8], lo[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) { hi[i] = f2bf(v[i]); lo[i] = f2bf(v[i] - bf2f((uint16_t)hi[i])); }
                    uint16_t* grp = (uint16_t*)j.dst + 2 * (d - (k & 15));
                    *reinterpret_cast<uint4*>(grp + (k & 15)) = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
                    *reinterpret_cast<uint4*>(grp + 16 + (k & 15)) = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
                }
            }
            if (j.dst_t && rows_n) {      // the transposed, tap-flipped layout from the same tile: n' = k (this tile's columns), k' = n (its rows)
                for (int item = tid; item < 9 * 128; item += 256) {
                    const int t = item >> 7, nn = (item & 127) >> 2, k8 = item & 3;
                    const int n = k0 + nn, k = n0 + 8 * k8;
                    if (n >= j.Kp || k >= j.Np) continue;
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = tf[8 * k8 + i][nn * 9 + (8 - t)];
                    const long long d = (((long long)(k / KCT) * 9 + t) * j.Kp + n) * KCT + (k % KCT);
                    if constexpr (__is_same(T, bf16_t)) {
                        *reinterpret_cast<uint4*>((uint16_t*)j.dst_t + d) =
                            make_uint4((unsigned)f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16), (unsigned)f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16),
                                       (unsigned)f2bf(v[4]) | ((unsigned)f2bf(v[5]) << 16), (unsigned)f2bf(v[6]) | ((unsigned)f2bf(v[7]) << 16));
                    } else {
                        unsigned hi[8], lo[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i) { hi[i] = f2bf(v[i]); lo[i] = f2bf(v[i] - bf2f((uint16_t)hi[i])); }
                        uint16_t* grp = (uint16_t*)j.dst_t + 2 * (d - (k & 15));
                        *reinterpret_cast<uint4*>(grp + (k & 15)) = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
                        *reinterpret_cast<uint4*>(grp + 16 + (k & 15)) = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
                    }
                }
            }
            return;
        }
    }
#endif
#pragma unroll
    for (int i = 0; i < PACK_TILE * PACK_TILE / 256; ++i) {
        const int idx = tid + 256 * i, a = idx & (PACK_TILE - 1), b = idx / PACK_TILE;
        const int nn = along_n ? a : b, kk = along_n ? b : a;
        const int n = n0 + nn, k = k0 + kk;
        int nl = -1, kl = -1;
        if (n < j.Np && k < j.Kp) {
            nl = phys2log(n, j.n_seg0, j.n_seg0p, j.N);
            kl = phys2log(k, j.k_seg0, j.k_seg0p, j.K);
        }
        const bool ok = nl >= 0 && kl >= 0;
        const float* src = j.src + (ok ? nl * j.sn + kl * j.sk : 0);
        for (int t = 0; t < j.T; ++t) tile[t][nn][kk] = ok ? src[(j.flip ? j.T - 1 - t : t) * j.st] : 0.f;      // unscaled: dst_t takes these
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PACK_TILE * PACK_TILE / 256; ++i) {
        const int idx = tid + 256 * i, kk = idx & (PACK_TILE - 1), nn = idx / PACK_TILE;
        const int n = n0 + nn, k = k0 + kk;
        if (n < j.Np && k < j.Kp) {
            const float ks = (j.kscale && phys2log(k, j.k_seg0, j.k_seg0p, j.K) >= 0) ? j.kscale[k] : 1.f;      // never a padded channel's entry
            for (int t = 0; t < j.T; ++t) {
                // element offset of (t, n, k) with k rounded down to its 16-channel group `kg` (+ k%16 added below)
                const long long d = j.kc > 0 ? (((long long)(k / j.kc) * j.T + t) * j.Np + n) * j.kc + (k % j.kc)
                                             : t * j.dt + n * j.dn + k * j.dk;
                if (j.dst_f32) ((float*)j.dst)[d] = tile[t][nn][kk] * ks;
                else if constexpr (__is_same(T, split_t)) {
                    // 4 bytes per element: every 16-channel group is stored as [16 x bf16 hi][16 x bf16 lo]
                    const float x = tile[t][nn][kk] * ks;
                    const uint16_t hi = f2bf(x);
                    uint16_t* grp = (uint16_t*)j.dst + 2 * (d - (k & 15));
                    grp[k & 15] = hi;
                    grp[16 + (k & 15)] = f2bf(x - bf2f(hi));
                } else st1<T>((T*)j.dst + d, tile[t][nn][kk] * ks);
            }
        }
    }
    if (j.dst_t && j.kc > 0) {      // transposed, tap-flipped second layout: lanes along n, the destination's contiguous index
#pragma unroll
        for (int i = 0; i < PACK_TILE * PACK_TILE / 256; ++i) {
            const int idx = tid + 256 * i, nn = idx & (PACK_TILE - 1), kk = idx / PACK_TILE;
            const int n = n0 + nn, k = k0 + kk;
            if (n < j.Np && k < j.Kp) {
                for (int t = 0; t < j.T; ++t) {
                    const long long d = (((long long)(n / j.kc) * j.T + (j.T - 1 - t)) * j.Kp + k) * j.kc + (n % j.kc);
                    const float x = tile[t][nn][kk];
                    if constexpr (__is_same(T, split_t)) {
                        const uint16_t hi = f2bf(x);
                        uint16_t* grp = (uint16_t*)j.dst_t + 2 * (d - (n & 15));
                        grp[n & 15] = hi;
                        grp[16 + (n & 15)] = f2bf(x - bf2f(hi));
                    } else st1<T>((T*)j.dst_t + d, x);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ metrics
// arg-max over classes (first maximum wins, as torch.max / argmax) fused with the confusion-matrix histogram
// conf[K*t + p] += 1 for 0 <= t < K  (metrics.py:32-38).  pred is optional (int64 [B,H,W]).
__global__ void argmax_confusion_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                        long long* pred, unsigned long long* conf, int B, int K, int Kc, long long HW) {
    extern __shared__ unsigned int hist[];   // Kc*Kc
    for (int i = threadIdx.x; i < Kc * Kc; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const long long npix = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW, p = i - b * HW;
        const float* z = logits + b * K * HW + p;
        float best = z[0];
        int arg = 0;
        for (int k = 1; k < K; ++k) {
            const float v = z[k * HW];
            if (v > best) { best = v; arg = k; }
        }
        if (pred) pred[i] = arg;
        if (labels) {
            const long long t = labels[i];
            if (t >= 0 && t < Kc && arg < Kc) atomicAdd(&hist[(int)t * Kc + arg], 1u);      // Kc < K: predictions outside the matrix are dropped
        }
    }
    __syncthreads();
    if (conf)
        for (int i = threadIdx.x; i < Kc * Kc; i += blockDim.x)
            if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}

// ------------------------------------------------------------------------------------------------ data path
// the reference's per-sample CPU pipeline
//   image: transforms.Pad(10) -> CenterCrop(h,w) -> ToTensor -> Normalize(0.5,0.5)        (main.py:18-23)
//   mask : Pad(10) -> CenterCrop(h,w) -> voc.to_mask (per-pixel Python loop over a 22-colour palette; void -> 0)
//                                                                                     (datasets/voc.py:56-72,140-142)
// as one kernel on interleaved uint8 RGB inputs.  Pad fills with 0 (torchvision default); CenterCrop of an image
// smaller than the crop pads with 0 as torchvision.transforms.functional.center_crop does.  (oy, ox) = position of the
// padded-and-cropped window's origin inside the source image (may be negative), computed on the host.
__constant__ unsigned int c_voc_palette[22] = {
    0x000000, 0x800000, 0x008000, 0x808000, 0x000080, 0x800080, 0x008080, 0x808080, 0x400000, 0xC00000, 0x408000,
    0xC08000, 0x400080, 0xC00080, 0x408080, 0xC08080, 0x004000, 0x804000, 0x00C000, 0x80C000, 0x004080, 0xE0E0C0};

__global__ void voc_prepare_kernel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ mask,
                                   float* image_out, long long* label_out, int Hs, int Ws, int oy, int ox, int h, int w,
                                   unsigned int* bad) {
    const int n = h * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int y = i / w, x = i - y * w;
        const int sy = y + oy, sx = x + ox;
        const bool in = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws;
        if (image_out) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = in ? (float)img[((long long)sy * Ws + sx) * 3 + c] / 255.f : 0.f;   // ToTensor
                image_out[(long long)c * n + i] = (v - 0.5f) / 0.5f;                                 // Normalize(0.5, 0.5)
            }
        }
        if (label_out) {
            unsigned int key = 0;
            if (in) {
                const unsigned char* m = mask + ((long long)sy * Ws + sx) * 3;
                key = ((unsigned int)m[0] << 16) | ((unsigned int)m[1] << 8) | m[2];
            }
            int cls = -1;
#pragma unroll
            for (int k = 0; k < 22; ++k) cls = (cls < 0 && c_voc_palette[k] == key) ? k : cls;
            if (cls == 21) cls = 0;                      // void -> background (voc.py:67-68)
            if (cls < 0) { atomicAdd(bad, 1u); cls = 0; }   // the reference raises ValueError (list.index): reported to the host
            label_out[i] = cls;
        }
    }
}

// labels [N,H,W] int64 -> RGB [N,3,H,W] float64-compatible values as float (datasets/voc.py:74-89 to_rgb), classes >= 22 -> 0
__global__ void label_to_rgb_kernel(const long long* __restrict__ labels, float* rgb, long long n_img, long long hw) {
    const long long n = n_img * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / hw, p = i - b * hw;
        const long long l = labels[i];
        const unsigned int key = (l >= 0 && l < 22) ? c_voc_palette[l] : 0u;
        rgb[(b * 3 + 0) * hw + p] = (float)((key >> 16) & 255u);
        rgb[(b * 3 + 1) * hw + p] = (float)((key >> 8) & 255u);
        rgb[(b * 3 + 2) * hw + p] = (float)(key & 255u);
    }
}

// p *= *scale unless *scale == 1 (wave-uniform early exit: no memory traffic).  loss.backward() hands the loss function an
// upstream gradient of exactly 1 as a DEVICE scalar; testing it on the device avoids both a host sync and a 176-MB pass.
__global__ void scale_by_dev_kernel(float* p, long long n, const float* __restrict__ scale) {
    const float v = *scale;
    if (v == 1.f) return;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] *= v;
}

// ... the same for an NHWC tensor of a compute dtype (the second copy of d logits the fused loss writes), 8-channel groups; with p32 != NULL
// the fp32 tensor is scaled by the same launch (both copies of d logits in one)
template <typename T>
__global__ void scale_by_dev_t_kernel(T* p, long long ngroups, const float* __restrict__ scale, float* p32, long long n32) {
    const float v = *scale;
    if (v == 1.f) return;
    if (p32)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n32; i += (long long)gridDim.x * blockDim.x) p32[i] *= v;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < ngroups; i += (long long)gridDim.x * blockDim.x) {
        float t[8];
        Vec8<T>::load(p + i * 8, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] *= v;
        Vec8<T>::store(p + i * 8, t);
    }
}

// Rehearsal aid (tools/cu_steal.py, tests): `gridDim.x` workgroups that each keep one CU to themselves for `ticks`
// 100-MHz ticks -- 96 KB of LDS per workgroup means at most one per CU and no room beside it for the 120-160-KB MFMA
// workgroups of this library -- the way an RCCL channel workgroup holds a CU during a collective.  Every wave exits at the
// deadline; nothing is read or written.
__global__ void __launch_bounds__(256) hold_cus_kernel(unsigned long long ticks, unsigned int* sink) {
    __shared__ unsigned int pad[96 * 1024 / 4];
    if (threadIdx.x == 0) pad[0] = 1u;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
    if (ticks == ~0ull && sink) sink[0] = pad[threadIdx.x];       // never true: keeps the LDS allocation alive
}

// Calibration loop for bench.py: the rate the matrix pipes SUSTAIN on pseudo-random operands (registers only, one wave per SIMD, every CU).
// bf16 MFMA loops on real data are power-limited on MI355X -- 1.7-1.9 PFLOP/s against the 2.5 PFLOP/s the clock-times-width peak promises
// (tools/ubench/mfma_shapes.hip) -- so a kernel's fraction of the nominal peak understates how close to the attainable rate it runs.
__device__ inline unsigned mix32(unsigned x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
template <bool BF16>
__global__ void __launch_bounds__(256) mfma_rate_kernel(float* sink, int iters) {
    uint4 a[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned hsh = mix32(threadIdx.x * 64u + j * 8u + e + blockIdx.x * 7919u);
            const float v = ((int)(hsh & 0xffffu) - 32768) * (1.f / 32768.f);
            w[e] = BF16 ? (unsigned)f2bf(v) | ((unsigned)f2bf(-v * 0.37f) << 16) : __float_as_uint(v);
        }
        a[j] = make_uint4(w[0], w[1], w[2], w[3]);
        b[j] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u)              // 32 MFMAs per iteration and wave
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (BF16) mma_bf16(a[(i + u) & 3], b[(j + 2 + u) & 3], acc[i][j]);
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[(i + u) & 3].x), __uint_as_float(b[(j + 2 + u) & 3].y), acc[i][j], 0, 0, 0);
                }
    }
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) t += acc[i][j][e];
    sink[blockIdx.x * 256 + threadIdx.x] = t;
}

// gradient exchange in bf16 (ddp.GradSync(grad_dtype='bf16'), BASELINE.json configs[2]/[4] "bf16 DDP"): a bucket of the flat
// fp32 gradient buffer is rounded to bf16 (rne) for the all-reduce and widened back afterwards.  A bucket starts at an
// arbitrary element of the flat buffer: `head` leading elements are converted one by one, the aligned body 8 per thread and
// pass (the bf16 buffer is placed at the same element phase, checked on entry), then the tail.
__global__ void __launch_bounds__(256) f32_to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, long long n, int head) {
    const long long nb = n - head, nv = nb >> 3;
    const float* sb = src + head;
    uint16_t* db = dst + head;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const float4 a = reinterpret_cast<const float4*>(sb)[2 * i], b = reinterpret_cast<const float4*>(sb)[2 * i + 1];
        reinterpret_cast<uint4*>(db)[i] = make_uint4(pack2bf(a.x, a.y), pack2bf(a.z, a.w), pack2bf(b.x, b.y), pack2bf(b.z, b.w));
    }
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < head) dst[threadIdx.x] = f2bf(src[threadIdx.x]);
        if ((long long)threadIdx.x < (nb & 7)) db[(nv << 3) + threadIdx.x] = f2bf(sb[(nv << 3) + threadIdx.x]);
    }
}
__global__ void __launch_bounds__(256) bf16_to_f32_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, long long n, int head) {
    const long long nb = n - head, nv = nb >> 3;
    const uint16_t* sb = src + head;
    float* db = dst + head;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
        const uint4 u = reinterpret_cast<const uint4*>(sb)[i];
        reinterpret_cast<float4*>(db)[2 * i] = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                                                           __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
        reinterpret_cast<float4*>(db)[2 * i + 1] = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u),
                                                               __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u));
    }
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < head) dst[threadIdx.x] = bf2f(src[threadIdx.x]);
        if ((long long)threadIdx.x < (nb & 7)) db[(nv << 3) + threadIdx.x] = bf2f(sb[(nv << 3) + threadIdx.x]);
    }
}

__global__ void fill_kernel(float* p, long long n, float v) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

}  // namespace clamd

using namespace clamd;

int clamd_launch_pack(const void* jobs_dev, int njobs, int total_blocks, int dtype, const FoldBias* fold, hipStream_t stream) {
    if (njobs <= 0 || total_blocks <= 0) return clamd_fail("pack: empty job table");
    const FoldBias f = fold ? *fold : FoldBias{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 9};
    const dim3 grid(total_blocks + (fold ? fold->Cout_p : 0));
    if (dtype == CLAMD_BF16)
        hipLaunchKernelGGL(pack_kernel<bf16_t>, grid, dim3(256), 0, stream, (const PackJob*)jobs_dev, njobs, total_blocks, f);
    else if (dtype == CLAMD_F32)
        hipLaunchKernelGGL(pack_kernel<float>, grid, dim3(256), 0, stream, (const PackJob*)jobs_dev, njobs, total_blocks, f);
    else if (dtype == CLAMD_SPLIT)
        hipLaunchKernelGGL(pack_kernel<split_t>, grid, dim3(256), 0, stream, (const PackJob*)jobs_dev, njobs, total_blocks, f);
    else return clamd_fail("pack: bad dtype");
    return clamd_check_launch("pack");
}

extern "C" {

const char* clamd_last_error(void) { return g_err; }
int clamd_version(void) { return 100; }
int clamd_sizeof_pack_job(void) { return (int)sizeof(PackJob); }
int clamd_pack_tile(void) { return PACK_TILE; }
int clamd_bn_bwd_nsums(void) { return 5; }

int clamd_pack(const void* jobs_dev, int njobs, int total_blocks, int dtype, void* stream) {
    return clamd_launch_pack(jobs_dev, njobs, total_blocks, dtype, nullptr, (hipStream_t)stream);
}

int clamd_scale_by_device_scalar_nhwc(void* p, long long n, int dtype, const float* scale_dev, float* also_f32, long long n_f32, void* stream) {
    if (n <= 0 || n % 8 || !scale_dev || !p || (also_f32 && n_f32 <= 0)) return clamd_fail("scale_by_device_scalar_nhwc: bad arguments (n must be a multiple of 8 channels)");
    if (int e = clamd_check_split(dtype, p, 16)) return e;
    long long g = (n / 8 + 255) / 256;
    if (g > 4096) g = 4096;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CLAMD_BF16) hipLaunchKernelGGL(scale_by_dev_t_kernel<bf16_t>, dim3((unsigned)g), dim3(256), 0, s, (bf16_t*)p, n / 8, scale_dev, also_f32, n_f32);
    else if (dtype == CLAMD_F32) hipLaunchKernelGGL(scale_by_dev_t_kernel<float>, dim3((unsigned)g), dim3(256), 0, s, (float*)p, n / 8, scale_dev, also_f32, n_f32);
    else if (dtype == CLAMD_SPLIT) hipLaunchKernelGGL(scale_by_dev_t_kernel<split_t>, dim3((unsigned)g), dim3(256), 0, s, (split_t*)p, n / 8, scale_dev, also_f32, n_f32);
    else return clamd_fail("scale_by_device_scalar_nhwc: bad dtype");
    return clamd_check_launch("scale_by_device_scalar_nhwc");
}

int clamd_argmax_confusion(const float* logits, const long long* labels, long long* pred, unsigned long long* conf,
                           int B, int K, int Kc, int H, int W, void* stream) {
    if (K < 1 || Kc < 1 || Kc > 64) return clamd_fail("argmax_confusion: bad class counts");
    const long long npix = (long long)B * H * W;
    int g = (int)((npix + 255) / 256);
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(argmax_confusion_kernel, dim3(g), dim3(256), Kc * Kc * sizeof(unsigned int), (hipStream_t)stream,
                       logits, labels, pred, conf, B, K, Kc, (long long)H * W);
    return clamd_check_launch("argmax_confusion");
}

int clamd_voc_prepare(const unsigned char* img_rgb, const unsigned char* mask_rgb, float* image_out, long long* label_out,
                      int Hs, int Ws, int oy, int ox, int h, int w, unsigned int* bad_count, void* stream) {
    if ((!image_out && !label_out) || h <= 0 || w <= 0 || Hs <= 0 || Ws <= 0) return clamd_fail("voc_prepare: bad arguments");
    if ((image_out && !img_rgb) || (label_out && (!mask_rgb || !bad_count))) return clamd_fail("voc_prepare: missing input");
    int g = (h * w + 255) / 256;
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(voc_prepare_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, img_rgb, mask_rgb, image_out, label_out,
                       Hs, Ws, oy, ox, h, w, bad_count);
    return clamd_check_launch("voc_prepare");
}

int clamd_label_to_rgb(const long long* labels, float* rgb, long long n_img, long long hw, void* stream) {
    long long n = n_img * hw;
    int g = (int)((n + 255) / 256);
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(label_to_rgb_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, labels, rgb, n_img, hw);
    return clamd_check_launch("label_to_rgb");
}

int clamd_scale_by_device_scalar(float* p, long long n, const float* scale_dev, void* stream) {
    if (n <= 0 || !scale_dev) return clamd_fail("scale_by_device_scalar: bad arguments");
    long long g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(scale_by_dev_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, p, n, scale_dev);
    return clamd_check_launch("scale_by_device_scalar");
}

long long clamd_debug_mfma_rate(int dtype, int iters, float* sink_65536, void* stream) {
    if (iters < 1 || iters > (1 << 20) || !sink_65536) { clamd_fail("debug_mfma_rate: 1..2^20 iterations and a sink of 65536 floats"); return -1; }
    if (dtype == CLAMD_F32) hipLaunchKernelGGL(mfma_rate_kernel<false>, dim3(256), dim3(256), 0, (hipStream_t)stream, sink_65536, iters);
    else hipLaunchKernelGGL(mfma_rate_kernel<true>, dim3(256), dim3(256), 0, (hipStream_t)stream, sink_65536, iters);
    if (clamd_check_launch("debug_mfma_rate")) return -1;
    return 256ll * 4 * iters * 32 * (dtype == CLAMD_F32 ? 4096 : 32768);      // FLOP of the launch
}

int clamd_hold_cus(int ncus, int usec, void* stream) {
    if (ncus < 1 || ncus > 256 || usec < 1 || usec > 2000000) return clamd_fail("hold_cus: 1..256 CUs for 1..2000000 us");
    hipLaunchKernelGGL(hold_cus_kernel, dim3(ncus), dim3(256), 0, (hipStream_t)stream, (unsigned long long)usec * 100ull, (unsigned int*)nullptr);
    return clamd_check_launch("hold_cus");
}
int clamd_debug_hold_cus(int ncus, int usec, void* stream) { return clamd_hold_cus(ncus, usec, stream); }

int clamd_fill_f32(float* p, long long n, double v, void* stream) {
    int g = (int)((n + 255) / 256);
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(fill_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, p, n, (float)v);
    return clamd_check_launch("fill");
}

// leading elements up to the first 32-byte boundary of the fp32 side; the bf16 side must sit at the same element phase
static int bf16_head(const void* f32, const void* bf16, long long n, int* head) {
    const unsigned long long a = (unsigned long long)f32, b = (unsigned long long)bf16;
    if ((a & 3ull) || (b & 1ull)) return -1;
    if (((a >> 2) & 7ull) != ((b >> 1) & 7ull)) return -1;
    const int h = (int)((8 - ((a >> 2) & 7ull)) & 7ull);
    *head = (long long)h < n ? h : (int)n;
    return 0;
}

int clamd_f32_to_bf16(const float* src, void* dst, long long n, void* stream) {
    if (n <= 0 || !src || !dst) return clamd_fail("f32_to_bf16: bad arguments");
    int head = 0;
    if (bf16_head(src, dst, n, &head)) return clamd_fail("f32_to_bf16: the bf16 buffer must sit at the fp32 buffer's element phase ((addr / elem size) % 8)");
    long long g = (((n - head) >> 3) + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, (uint16_t*)dst, n, head);
    return clamd_check_launch("f32_to_bf16");
}

int clamd_bf16_to_f32(const void* src, float* dst, long long n, void* stream) {
    if (n <= 0 || !src || !dst) return clamd_fail("bf16_to_f32: bad arguments");
    int head = 0;
    if (bf16_head(dst, src, n, &head)) return clamd_fail("bf16_to_f32: the bf16 buffer must sit at the fp32 buffer's element phase ((addr / elem size) % 8)");
    long long g = (((n - head) >> 3) + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, dst, n, head);
    return clamd_check_launch("bf16_to_f32");
}

}  // extern "C"
