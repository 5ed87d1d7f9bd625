// Pseudo-labelling of the old classes in the task step (build-defined, parity unpinned: the reference has no continual-learning code; the
// classification half of PLOP, Douillard et al., CVPR 2021, section 3.2, as include/clamd.h restates it).
//   clamd_pseudo_entropy_hist   calibration: histogram of the old model's normalised entropy over the background pixels, per arg-max class
//   clamd_pseudo_label          the per-step relabelling: confident background pixels take the old model's class, the others ignore_index;
//                               per-image counts and the adaptive factor nu_b
// The step's loss, clamd_ce_fwd_bwd_weighted, is in loss.hip.
// Both are one pass over the c_old old-model logits and the labels: c*, u and the decision come from the soft-max state (e_k = exp(zo_k - max),
// sum e) in registers.  ce4_kernel's shape (loss.hip) throughout: NPX = 4 consecutive pixels per thread with 16-byte logit and 32-byte label
// accesses (four consecutive pixels share an image when H * W % 4 == 0), NPX = 1 the same arithmetic for other sizes.
#include <math.h>
#include <stdio.h>
#include "common.hip.h"
#include "ce_common.hip.h"
#include "clamd_internal.h"

namespace clamd {

// c* (lowest index of the maximum: a later class must be strictly larger) and u = -(sum_k q_k ln q_k) / ln(c_old) of NPX pixels.  With
// d_k = zo_k - max, e_k = exp(d_k), s = sum e_k:  ln q_k = d_k - ln s, so  -sum q_k ln q_k = ln s - (sum e_k d_k) / s.  A class whose e_k
// underflowed adds 0 (its q_k ln q_k -> 0), also when zo_k = -inf.  inv_lnc = 1 / ln(c_old), 0 for c_old == 1 (u = 0).
template <int KOLD, int NPX>
__device__ inline void pseudo_verdict(const float* __restrict__ zo, long long HW, int c_old, float inv_lnc, int (&arg)[4], float (&u)[4]) {
    float4 o[KOLD];
#pragma unroll
    for (int k = 0; k < KOLD; ++k)
        if (k < c_old) o[k] = ce_ldpx<NPX>(zo + k * HW);
    float4 mo = o[0];
    CE_PX arg[c] = 0;
#pragma unroll
    for (int k = 1; k < KOLD; ++k)
        if (k < c_old) CE_PX {
            const float v = ce_at(o[k], c);
            const bool up = v > ce_at(mo, c);
            ce_at(mo, c) = up ? v : ce_at(mo, c);
            arg[c] = up ? k : arg[c];
        }
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = s;
#pragma unroll
    for (int k = 0; k < KOLD; ++k)
        if (k < c_old) CE_PX {
            const float d = ce_at(o[k], c) - ce_at(mo, c);
            const float e = expf(d);
            ce_at(s, c) += e;
            ce_at(t, c) += e > 0.f ? e * d : 0.f;
        }
    CE_PX u[c] = (logf(ce_at(s, c)) - ce_at(t, c) / ce_at(s, c)) * inv_lnc;
}

// bin(u) = min(NB - 1, floor(u * NB)).  Only a u >= 0 is converted: one that rounding left a hair below 0, or a NaN (a NaN logit, or every
// logit -inf), goes to bin 0, so the index is inside the row by construction.
__device__ inline int pseudo_bin(float u, int nbins) {
    const float r = u >= 0.f ? fminf(floorf(u * (float)nbins), (float)(nbins - 1)) : 0.f;
    return (int)r;
}

// hist[c*][bin(u)] += 1 over the pixels with label 0: a histogram per workgroup in LDS (integer atomics), added to the int64 one in memory
// with one integer atomic per non-empty bin.  Threads without a candidate pixel do not read the logits.
template <int KOLD, int NPX>
__global__ void __launch_bounds__(256) pseudo_hist_kernel(const float* __restrict__ old_logits, int K_old_total, int c_old, float inv_lnc,
                                                          const long long* __restrict__ labels, unsigned long long* hist, int nbins, int B,
                                                          long long HW) {
    extern __shared__ unsigned int lh[];      // [c_old][nbins]
    const int nh = c_old * nbins;
    for (int i = threadIdx.x; i < nh; i += 256) lh[i] = 0;
    __syncthreads();
    const long long nq = (long long)B * HW / NPX;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += (long long)gridDim.x * 256) {
        const long long pix = NPX * i, b = pix / HW, p = pix - b * HW;
        long long lab[4];
        ce_ld_labels<NPX>(labels, pix, lab);
        bool any = false;
        CE_PX any |= lab[c] == 0;
        if (!any) continue;
        int arg[4];
        float u[4];
        pseudo_verdict<KOLD, NPX>(old_logits + b * K_old_total * HW + p, HW, c_old, inv_lnc, arg, u);
        CE_PX if (lab[c] == 0) atomicAdd(&lh[arg[c] * nbins + pseudo_bin(u[c], nbins)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += 256)
        if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
}

// labels_out and counts[b] = {n_bg, n_acc}.  The counts of a wave whose lanes sit in one image (the usual case: lanes hold consecutive
// pixels) are added with shuffles, {n_bg, n_acc} packed in the two halves of a word (<= 256 each), and reach the workgroup's LDS counters
// through lane 0; a wave that straddles two images adds per lane.  The trip count is uniform (the shuffles need every lane).
template <int KOLD, int NPX>
__global__ void __launch_bounds__(256) pseudo_label_kernel(const float* __restrict__ old_logits, int K_old_total, int c_old, float inv_lnc,
                                                           const long long* __restrict__ labels_in, const float* __restrict__ thresholds,
                                                           long long* __restrict__ labels_out, unsigned int* counts, int B, long long HW,
                                                           long long ignore_index) {
    extern __shared__ unsigned int lc[];      // [B][2]
    __shared__ float tau[32];
    for (int i = threadIdx.x; i < 2 * B; i += 256) lc[i] = 0;
    if ((int)threadIdx.x < c_old) tau[threadIdx.x] = thresholds[threadIdx.x];
    __syncthreads();
    const long long nq = (long long)B * HW / NPX;
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256; base < nq; base += (long long)gridDim.x * 256) {
        const long long i = base + threadIdx.x;
        const bool live = i < nq;
        const long long pix = NPX * (live ? i : nq - 1), b = pix / HW, p = pix - b * HW;
        long long lab[4];
        ce_ld_labels<NPX>(labels_in, pix, lab);
        bool any = false;
        CE_PX any |= lab[c] == 0;
        unsigned int packed = 0;
        if (live && any) {
            int arg[4];
            float u[4];
            pseudo_verdict<KOLD, NPX>(old_logits + b * K_old_total * HW + p, HW, c_old, inv_lnc, arg, u);
            CE_PX if (lab[c] == 0) {
                const bool acc = u[c] < tau[arg[c]];
                lab[c] = acc ? (long long)arg[c] : ignore_index;
                packed += acc ? 0x10001u : 1u;
            }
        }
        if (live) {
            if constexpr (NPX == 4) *reinterpret_cast<longlong4*>(labels_out + pix) = *reinterpret_cast<const longlong4*>(lab);
            else labels_out[pix] = lab[0];
        }
        const int bi = (int)b;
        if (__shfl(bi, 0) == __shfl(bi, 63)) {      // b does not decrease along the lanes: equal ends = one image
            unsigned int w = packed;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o);
            if (lane == 0 && w) { atomicAdd(&lc[2 * bi], w & 0xffffu); atomicAdd(&lc[2 * bi + 1], w >> 16); }
        } else if (packed) {
            atomicAdd(&lc[2 * bi], packed & 0xffffu);
            atomicAdd(&lc[2 * bi + 1], packed >> 16);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * B; i += 256)
        if (lc[i]) atomicAdd(&counts[i], lc[i]);
}

// nu_b = n_bg ? max(min_factor, float(n_acc) / float(n_bg)) : 1
__global__ void pseudo_weight_kernel(const unsigned int* __restrict__ counts, float* __restrict__ w, float min_factor, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        const unsigned int nbg = counts[2 * b], nacc = counts[2 * b + 1];
        w[b] = nbg ? fmaxf(min_factor, (float)nacc / (float)nbg) : 1.f;
    }
}

}  // namespace clamd

using namespace clamd;

// what the two old-model passes share: the argument checks, whether the four-pixel form applies, the grid
static int pseudo_common(const char* what, const float* old_logits, int K_old_total, int c_old, const long long* labels, const void* labels_out,
                         int B, int H, int W, bool* four, float* inv_lnc) {
    static thread_local char msg[160];
#define PSEUDO_FAIL(text_) do { snprintf(msg, sizeof(msg), "%s: %s", what, text_); return clamd_fail(msg); } while (0)
    if (!old_logits || !labels || B <= 0 || H <= 0 || W <= 0) PSEUDO_FAIL("null pointer or empty shape");
    if (c_old < 1 || c_old > 32) PSEUDO_FAIL("c_old must be in [1, 32]");
    if (c_old > K_old_total) PSEUDO_FAIL("c_old exceeds the old model's class count K_old_total");
    if (((size_t)old_logits % 4) || ((size_t)labels % 8) || ((size_t)labels_out % 8)) PSEUDO_FAIL("misaligned tensor");
#undef PSEUDO_FAIL
    const long long HW = (long long)H * W;
    *four = HW % 4 == 0 && ((size_t)old_logits % 16) == 0 && ((size_t)labels % 32) == 0 && ((size_t)labels_out % 32) == 0;
    *inv_lnc = c_old > 1 ? (float)(1.0 / log((double)c_old)) : 0.f;
    return 0;
}

extern "C" {

int clamd_pseudo_entropy_hist(const float* old_logits, int K_old_total, int c_old, const long long* labels, long long* hist, int nbins,
                              int B, int H, int W, void* stream) {
    bool four;
    float inv_lnc;
    if (int e = pseudo_common("pseudo_entropy_hist", old_logits, K_old_total, c_old, labels, nullptr, B, H, W, &four, &inv_lnc)) return e;
    if (!hist || ((size_t)hist % 8)) return clamd_fail("pseudo_entropy_hist: hist must be an 8-byte aligned int64 [c_old, nbins] tensor");
    if (nbins < 1 || (long long)c_old * nbins > 8192) return clamd_fail("pseudo_entropy_hist: nbins must be >= 1 and c_old * nbins <= 8192 (the workgroup's histogram lives in LDS)");
    const long long HW = (long long)H * W, nq = (long long)B * HW / (four ? 4 : 1);
    int g = (int)((nq + 255) / 256);
    if (g > 1024) g = 1024;
    const size_t lds = (size_t)c_old * nbins * sizeof(unsigned int);
    hipStream_t s = (hipStream_t)stream;
#define PH(KO_, NPX_) hipLaunchKernelGGL((pseudo_hist_kernel<KO_, NPX_>), dim3(g), dim3(256), lds, s, old_logits, K_old_total, c_old, inv_lnc, labels, (unsigned long long*)hist, nbins, B, HW)
    if (!four) PH(32, 1);
    else if (c_old <= 8) PH(8, 4); else if (c_old <= 16) PH(16, 4); else if (c_old <= 24) PH(24, 4); else PH(32, 4);
#undef PH
    return clamd_check_launch("pseudo_entropy_hist");
}

int clamd_pseudo_label(const float* old_logits, int K_old_total, int c_old, const long long* labels_in, const float* thresholds,
                       long long* labels_out, unsigned int* counts, float* image_weight, double min_factor, int B, int H, int W,
                       long long ignore_index, void* stream) {
    bool four;
    float inv_lnc;
    if (int e = pseudo_common("pseudo_label", old_logits, K_old_total, c_old, labels_in, labels_out, B, H, W, &four, &inv_lnc)) return e;
    if (!thresholds || !labels_out || !counts) return clamd_fail("pseudo_label: null thresholds, labels_out or counts");
    if (B > 4096) return clamd_fail("pseudo_label: at most 4096 images per call (the workgroup's per-image counters live in LDS)");
    if (!(min_factor >= 0.0) || !(min_factor <= 3.0e38)) return clamd_fail("pseudo_label: min_factor must be finite and >= 0");
    const long long HW = (long long)H * W, nq = (long long)B * HW / (four ? 4 : 1);
    int g = (int)((nq + 255) / 256);
    if (g > 2048) g = 2048;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * 2 * sizeof(unsigned int), s) != hipSuccess) return clamd_fail("pseudo_label: memset failed");
    const size_t lds = (size_t)B * 2 * sizeof(unsigned int);
#define PL(KO_, NPX_) hipLaunchKernelGGL((pseudo_label_kernel<KO_, NPX_>), dim3(g), dim3(256), lds, s, old_logits, K_old_total, c_old, inv_lnc, labels_in, thresholds, labels_out, counts, B, HW, ignore_index)
    if (!four) PL(32, 1);
    else if (c_old <= 8) PL(8, 4); else if (c_old <= 16) PL(16, 4); else if (c_old <= 24) PL(24, 4); else PL(32, 4);
#undef PL
    if (image_weight)
        hipLaunchKernelGGL(pseudo_weight_kernel, dim3((B + 255) / 256), dim3(256), 0, s, counts, image_weight, (float)min_factor, B);
    return clamd_check_launch("pseudo_label");
}

}  // extern "C"
