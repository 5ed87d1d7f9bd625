// Pseudo-labelling of the old classes in the task step (build-defined, parity unpinned: the reference has no continual-learning code; the
// classification half of PLOP, Douillard et al., CVPR 2021, section 3.2, as include/clamd.h restates it).
//   clamd_pseudo_entropy_hist   calibration: histogram of the old model's normalised entropy over the background pixels, per arg-max class
//   clamd_pseudo_label          the per-step relabelling: confident background pixels take the old model's class, the others ignore_index;
//                               per-image counts and the adaptive factor nu_b
//   clamd_ce_fwd_bwd_weighted   the cross-entropy of clamd_ce_fwd_bwd_counted with the image's nu_b on every pixel's term
// The first two are one pass over the c_old old-model logits and the labels: c*, u and the decision come from the soft-max state
// (e_k = exp(zo_k - max), sum e) in registers.  ce4_kernel's shape throughout: NPX = 4 consecutive pixels per thread with 16-byte logit and
// 32-byte label accesses (four consecutive pixels share an image when H * W % 4 == 0), NPX = 1 the same arithmetic for other sizes.
#include <math.h>
#include <stdio.h>
#include "common.hip.h"
#include "ce_common.hip.h"
#include "clamd_internal.h"

namespace clamd {

#define CE_PX _Pragma("unroll") for (int c = 0; c < NPX; ++c)

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

template <int NPX> __device__ inline void pseudo_ld_labels(const long long* __restrict__ labels, long long pix, long long (&lab)[4]) {
    if constexpr (NPX == 4) *reinterpret_cast<longlong4*>(lab) = *reinterpret_cast<const longlong4*>(labels + pix);
    else lab[0] = labels[pix];
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
        pseudo_ld_labels<NPX>(labels, pix, lab);
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
        pseudo_ld_labels<NPX>(labels_in, pix, lab);
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

// ce4_kernel (misc.hip) with the image's weight: the same operations in the same order -- the maxima, one exponential per logit kept in the
// logit's register, the sequential sum, a thread's terms added pixel by pixel, the partial rows -- with nu_b multiplied in as ONE fp32
// factor, into the pixel's loss term and into gs = grad_scale / max(N, 1).  nu_b == 1.0f changes no bit of either.  A kernel of its own,
// so that ce4_kernel's instantiations stay what they were.  NPX = 1: one pixel per thread, any size or alignment.
template <int KMAX, int NPX, typename NT>
__global__ void __launch_bounds__(256) ce4w_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                   const float* __restrict__ image_weight, float* __restrict__ dlogits,
                                                   float* __restrict__ partial, int B, int K, long long HW, long long ignore_index,
                                                   float grad_scale, NT* dl_nhwc, int dl_ldc, const unsigned int* __restrict__ count_rows) {
    __shared__ float red[4];
    __shared__ unsigned int cnt_tmp[4];
    const long long nq = (long long)B * HW / NPX;
    const unsigned int nv = ce_count_total(count_rows, 0, cnt_tmp);
    const float gs = grad_scale / (float)max(nv, 1u);
    float ce_sum = 0.f;
    constexpr bool XCH = NPX == 4 && __is_same(NT, bf16_t) && CE_EXCHANGE;
    __shared__ uint4 xbuf[XCH ? 4 : 1][XCH ? 1024 : 1];
    for (long long base = (long long)blockIdx.x * blockDim.x; base < nq; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool live = i < nq;                                    // the trip count is block-uniform (the exchange has barriers)
        if (!XCH && !live) continue;
        const long long pix = NPX * (live ? i : nq - 1), b = pix / HW, p = pix - b * HW;
        const float nu = image_weight[b];
        const float gw = gs * nu;
        const float* z = logits + b * K * HW + p;
        float4 v[KMAX];
        float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                v[k] = ce_ldpx<NPX>(z + k * HW);
                CE_PX ce_at(mx, c) = fmaxf(ce_at(mx, c), ce_at(v[k], c));
            }
        long long lab[4];
        pseudo_ld_labels<NPX>(labels, pix, lab);
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f), picked = se;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) CE_PX {
                ce_at(picked, c) = lab[c] == k ? ce_at(v[k], c) : ce_at(picked, c);
                ce_at(v[k], c) = expf(ce_at(v[k], c) - ce_at(mx, c));
                ce_at(se, c) += ce_at(v[k], c);
            }
        bool ok[NPX];
        CE_PX ok[c] = lab[c] != ignore_index && lab[c] >= 0 && lab[c] < K;
        if (live) CE_PX {
            if (ok[c]) ce_sum += nu * (ce_at(mx, c) + logf(ce_at(se, c)) - ce_at(picked, c));
        }
        float r[NPX], h[NPX];
        CE_PX { r[c] = ok[c] ? gw / ce_at(se, c) : 0.f; h[c] = ok[c] ? gw : 0.f; }
        float* d = dlogits + b * K * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                CE_PX ce_at(g, c) = ce_at(v[k], c) * r[c] - (lab[c] == k ? h[c] : 0.f);
                if (live) {
                    if constexpr (NPX == 4) *reinterpret_cast<float4*>(d + k * HW) = g;
                    else d[k * HW] = g.x;
                }
                if constexpr (!__is_same(NT, ce_no_nhwc)) v[k] = g;
            }
        if constexpr (NPX == 4) ce_store_nhwc4<KMAX, NT, XCH>(v, K, dl_nhwc, dl_ldc, pix, base, nq, xbuf);
        else if constexpr (!__is_same(NT, ce_no_nhwc)) {
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {
                float t[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) t[j] = (cg * 8 + j < KMAX && cg * 8 + j < K) ? v[cg * 8 + j < KMAX ? cg * 8 + j : 0].x : 0.f;
                Vec8<NT>::store(dl_nhwc + pix * dl_ldc + cg * 8, t);
            }
        }
    }
    ce_sum = wave_sum(ce_sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ce_sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x + 0] = red[0] + red[1] + red[2] + red[3];
        partial[2 * blockIdx.x + 1] = 0.f;
    }
}
#undef CE_PX

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

int clamd_ce_fwd_bwd_weighted(const float* logits, const long long* labels, const float* image_weight, float* dlogits, void* dl_nhwc,
                              int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W,
                              long long ignore_index, double grad_scale, void* stream) {
    if (!logits || !labels || !dlogits || !loss3 || !workspace || B <= 0 || H <= 0 || W <= 0) return clamd_fail("ce_weighted: null pointer or empty shape");
    if (!image_weight) return clamd_fail("ce_weighted: image_weight (B floats) is required (clamd_ce_fwd_bwd_counted is the unweighted loss)");
    if (K < 1 || K > 32) return clamd_fail("ce_weighted: number of classes must be in [1, 32]");
    if (ws_bytes < clamd_ce_workspace_bytes()) return clamd_fail("ce: workspace too small");
    if (((size_t)logits % 4) || ((size_t)dlogits % 4) || ((size_t)image_weight % 4) || ((size_t)labels % 8)) return clamd_fail("ce_weighted: misaligned tensor");
    if (dl_nhwc) {
        if (dl_ldc < 32 || dl_ldc % 8 || ((size_t)dl_nhwc % 16)) return clamd_fail("ce_weighted: the NHWC copy needs a pitch >= 32 channels, a multiple of 8, and a 16-byte aligned base");
        if (dl_dtype != CLAMD_BF16 && dl_dtype != CLAMD_F32 && dl_dtype != CLAMD_SPLIT) return clamd_fail("ce_weighted: bad dtype");
        if (int e = clamd_check_split(dl_dtype, dl_nhwc, dl_ldc)) return e;
    }
    const long long HW = (long long)H * W, npix = (long long)B * HW;
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const unsigned int* rows = (const unsigned int*)(partial + 2 * 2048 + 4);
    const bool four = HW % 4 == 0 && ((size_t)logits % 16) == 0 && ((size_t)dlogits % 16) == 0 && ((size_t)labels % 32) == 0;
    int g = (int)(((four ? npix / 4 : npix) + 255) / 256);      // clamd_ce_fwd_bwd_counted's grid: the same partial rows
    if (g > 2048) g = 2048;
#define CEW(KM_, NPX_, T_) hipLaunchKernelGGL((ce4w_kernel<KM_, NPX_, T_>), dim3(g), dim3(256), 0, s, logits, labels, image_weight, dlogits, partial, B, K, HW, ignore_index, (float)grad_scale, (T_*)dl_nhwc, dl_ldc, rows)
#define CEWK(T_) do { if (!four) CEW(32, 1, T_); else if (K <= 8) CEW(8, 4, T_); else if (K <= 16) CEW(16, 4, T_); else if (K <= 24) CEW(24, 4, T_); else CEW(32, 4, T_); } while (0)
    if (!dl_nhwc) CEWK(ce_no_nhwc);
    else if (dl_dtype == CLAMD_BF16) CEWK(bf16_t);
    else if (dl_dtype == CLAMD_F32) CEWK(float);
    else CEWK(split_t);
#undef CEWK
#undef CEW
    clamd_ce_finalize_counted(partial, g, workspace, npix, loss3, s);
    return clamd_check_launch("ce_fwd_bwd_weighted");
}

}  // extern "C"
