// The per-pixel loss family: fused cross-entropy forward + backward and its build-defined continual-learning
// variants (A12: the distillation term, the unbiased class-incremental step, the per-image weight of the pseudo-label step).
//   clamd_ce_fwd_bwd            plain loss, any size; or + temperature distillation (ce_kernel, one pixel per thread)
//   clamd_ce_count              the {valid, bad} pixel counts as partial rows, for the three entry points below
//   clamd_ce_fwd_bwd_counted    the training-step form: four pixels per thread, d logits optionally a second time in NHWC
//   clamd_ce_fwd_bwd_weighted   the same with the image's factor nu_b on every pixel's term
//   clamd_ce_unbiased_fwd_bwd   unbiased cross-entropy + unbiased distillation
//   clamd_ce_class_fwd_bwd      class weights, label smoothing or the focal term (+ the image's factor); its own per-class count in front
// Every entry point: [count ->] one loss kernel (a {ce, kd} partial pair per workgroup) -> ce_finalize_kernel.
#include <math.h>
#include <stdio.h>
#include <type_traits>
#include "common.hip.h"
#include "ce_common.hip.h"
#include "clamd_internal.h"

namespace clamd {

// logits NCHW fp32 [B,K,H,W]; labels int64 [B,H,W].  nn.CrossEntropyLoss() (trainer.py:113): mean over pixels
// whose label != ignore_index.  Optional distillation (build-defined, parity unpinned):
//   + lam * mean_px KL( softmax(z_old[:, :c_old]/T) || softmax(z[:, :c_old]/T) )
// count[0] = pixels that take part in the mean (label != ignore_index and inside [0, K)); count[1] = pixels whose label is
// neither ignore_index nor a class -- torch's CrossEntropyLoss asserts on those; here they are left out of the loss and
// REPORTED (the host side exposes the counter, loss.py), so a label bug in a class split cannot hide.

// The caller's workspace, in 32-bit words: the loss kernel's partial pairs, the two totals (two spare words), the count rows.
constexpr int CE_MAX_BLOCKS = 2048;                            // grid cap of the loss kernels: one partial {ce, kd} pair each
constexpr int CE_COUNT_BLOCKS = 256;                           // workgroups of count_valid_rows_kernel: one partial {valid, bad} pair each
constexpr int CE_WS_TOTALS = 2 * CE_MAX_BLOCKS;                // {valid, bad} totals, written by ce_finalize_kernel
constexpr int CE_WS_ROWS = CE_WS_TOTALS + 4;
constexpr int CE_WS_WORDS = CE_WS_ROWS + 2 * CE_COUNT_BLOCKS;

// The count as one partial pair per workgroup (plain stores: no memset in front, no serialised atomics behind); the consumers add the
// CE_COUNT_BLOCKS pairs themselves (integers: any order gives the same sum).
__global__ void __launch_bounds__(256) count_valid_rows_kernel(const long long* __restrict__ labels, long long n, long long ignore_index,
                                                               int K, unsigned int* rows /* [CE_COUNT_BLOCKS][2] */) {
    unsigned int c = 0, bad = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long l = labels[i];
        const bool in = l >= 0 && l < K;
        c += (l != ignore_index && in) ? 1u : 0u;
        bad += (l != ignore_index && !in) ? 1u : 0u;
    }
    __shared__ unsigned int wsum[2][4];
    c = (unsigned int)wave_sum((float)c);   // <= 64 * iterations: exact in fp32 for the sizes used here
    bad = (unsigned int)wave_sum((float)bad);
    if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = c; wsum[1][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        rows[2 * blockIdx.x + 0] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        rows[2 * blockIdx.x + 1] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    }
}

// total of column `col` of those rows, by every thread of a 256-thread workgroup (through `tmp`, 4 words of LDS)
__device__ inline unsigned int ce_count_total(const unsigned int* __restrict__ rows, int col, unsigned int* tmp) {
    static_assert(CE_COUNT_BLOCKS == 256, "one row per thread");
    unsigned int v = rows[2 * threadIdx.x + col];
    v += __shfl_xor(v, 32); v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    return tmp[0] + tmp[1] + tmp[2] + tmp[3];
}

template <int KMAX>
__global__ void __launch_bounds__(256) ce_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                 const float* __restrict__ old_logits, int K_old_total, int c_old,
                                                 float inv_temp, float lam, float* __restrict__ dlogits,
                                                 float* __restrict__ partial, const unsigned int* __restrict__ count_rows,
                                                 int B, int K, long long HW, long long ignore_index, float grad_scale) {
    __shared__ unsigned int cnt_tmp[4];
    const long long npix = (long long)B * HW;
    const float inv_valid = 1.f / (float)max(ce_count_total(count_rows, 0, cnt_tmp), 1u);
    const float inv_npix = 1.f / (float)npix;
    float ce_sum = 0.f, kd_sum = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW, p = i - b * HW;
        const float* z = logits + b * K * HW + p;
        float v[KMAX];
        float mx = -INFINITY;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            v[k] = k < K ? z[k * HW] : -INFINITY;
            mx = fmaxf(mx, v[k]);
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) se += k < K ? expf(v[k] - mx) : 0.f;
        // log softmax_k = (z_k - max) - log(sum): the difference first.  z_k - (max + log(sum)) would round the log-sum-exp to an ulp of |max|
        // (2^-17 at logits near 100), a relative error of that size in the softmax of the largest logits
        const float lg = logf(se), lse = mx + lg;
        const long long lab = labels[i];
        const bool valid = lab != ignore_index && lab >= 0 && lab < K;
        float picked = 0.f;
        float g[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const float sm = k < K ? expf((v[k] - mx) - lg) : 0.f;
            const bool hit = valid && k == (int)lab;
            picked = hit ? v[k] : picked;
            g[k] = valid ? (sm - (hit ? 1.f : 0.f)) * inv_valid : 0.f;
        }
        if (valid) ce_sum += lse - picked;
        if (old_logits) {
            const float* zo = old_logits + b * K_old_total * HW + p;
            float o[KMAX];
            float mo = -INFINITY, mn = -INFINITY;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                o[k] = k < c_old ? zo[k * HW] * inv_temp : -INFINITY;
                mo = fmaxf(mo, o[k]);
                mn = fmaxf(mn, k < c_old ? v[k] * inv_temp : -INFINITY);
            }
            float so = 0.f, sn = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                so += k < c_old ? expf(o[k] - mo) : 0.f;
                sn += k < c_old ? expf(v[k] * inv_temp - mn) : 0.f;
            }
            const float lgo = logf(so), lgn = logf(sn);
            float kl = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < c_old) {
                    const float lp = (o[k] - mo) - lgo, lq = (v[k] * inv_temp - mn) - lgn;          // as above
                    const float pk = expf(lp);
                    kl += pk * (lp - lq);
                    g[k] += lam * inv_npix * inv_temp * (expf(lq) - pk);
                }
            kd_sum += kl;
        }
        float* d = dlogits + b * K * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) d[k * HW] = g[k] * grad_scale;
    }
    ce_block_pair<true>(wave_sum(ce_sum), wave_sum(kd_sum), partial);
}

struct ce_no_nhwc {};
#ifdef CE_NO_EXCHANGE      // A/B builds of the NHWC copy stored straight from the registers
#define CE_EXCHANGE false
#else
#define CE_EXCHANGE true
#endif
// The second copy of d logits of a lane's four consecutive pixels (v[k] = the gradient of class k), NHWC [pixel][dl_ldc] in dtype NT, channels
// K .. 31 zero.  XCH (bf16): through LDS, with two workgroup barriers -- every lane of the workgroup calls.
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
// ... and of a lane's one pixel (NPX = 1: v[k].x), straight from the registers
template <int KMAX, typename NT>
__device__ inline void ce_store_nhwc1(const float4 (&v)[KMAX], int K, NT* dl_nhwc, int dl_ldc, long long pix) {
    if constexpr (!__is_same(NT, ce_no_nhwc)) {
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = (cg * 8 + j < KMAX && cg * 8 + j < K) ? v[cg * 8 + j < KMAX ? cg * 8 + j : 0].x : 0.f;
            Vec8<NT>::store(dl_nhwc + pix * dl_ldc + cg * 8, t);
        }
    }
}

// The plain loss of the training step and, WEIGHTED, the pseudo-label step's: NPX = 4 consecutive pixels per thread (H * W % 4 == 0, so they
// share an image) -- 16-byte loads and stores, K * 16 bytes in flight per lane instead of K * 4 -- and ONE exponential per logit (e = exp(z - max)
// is kept in the logit's register; softmax = e / sum).  NPX = 1: the same arithmetic, one pixel per thread, for any size or alignment.
// NT != ce_no_nhwc: d logits is ALSO written as an NHWC tensor [pixel][ldc] of compute dtype NT (channels K .. 31 zero) -- the layout the 1x1
// head's data gradient reads, so the backward pass needs no NCHW -> NHWC conversion (88 + 67 MB at config 2 in bf16): a thread's four
// pixels are consecutive there too (4 x 64 bytes in bf16).
// WEIGHTED: the image's nu_b multiplied in as ONE fp32 factor, into the pixel's loss term and into gs = grad_scale / max(N, 1); every other
// operation is the unweighted one in the same order, so nu_b == 1.0f changes no bit.  Unweighted, the kernel takes no weight at all.
struct ce_no_weight {};
template <int KMAX, int NPX, typename NT, bool WEIGHTED>
__global__ void __launch_bounds__(256) ce4_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                  std::conditional_t<WEIGHTED, const float* __restrict__, ce_no_weight> image_weight,
                                                  float* __restrict__ dlogits, float* __restrict__ partial, int B, int K, long long HW,
                                                  long long ignore_index, float grad_scale, NT* dl_nhwc, int dl_ldc,
                                                  const unsigned int* __restrict__ count_rows) {
    __shared__ unsigned int cnt_tmp[4];
    const long long nq = (long long)B * HW / NPX;
    const unsigned int nv = ce_count_total(count_rows, 0, cnt_tmp);
    const float gs = grad_scale / (float)max(nv, 1u);
    float ce_sum = 0.f;
    constexpr bool XCH = NPX == 4 && __is_same(NT, bf16_t) && CE_EXCHANGE;      // NHWC copy through LDS: whole KBs per store instruction
    __shared__ uint4 xbuf[XCH ? 4 : 1][XCH ? 1024 : 1];
    for (long long base = (long long)blockIdx.x * blockDim.x; base < nq; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool live = i < nq;                                    // the trip count is block-uniform (the exchange below has barriers)
        if (!XCH && !live) continue;
        const long long pix = NPX * (live ? i : nq - 1), b = pix / HW, p = pix - b * HW;
        float nu = 1.f, gw = gs;
        if constexpr (WEIGHTED) { nu = image_weight[b]; gw = gs * nu; }
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
        ce_ld_labels<NPX>(labels, pix, lab);
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f), picked = se;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                CE_PX ce_at(picked, c) = lab[c] == k ? ce_at(v[k], c) : ce_at(picked, c);
                CE_PX ce_at(v[k], c) = expf(ce_at(v[k], c) - ce_at(mx, c));
                CE_PX ce_at(se, c) += ce_at(v[k], c);
            }
        bool ok[NPX];
        CE_PX ok[c] = lab[c] != ignore_index && lab[c] >= 0 && lab[c] < K;
        if (live) CE_PX {
            if (ok[c]) {
                const float t = ce_at(mx, c) + logf(ce_at(se, c)) - ce_at(picked, c);
                if constexpr (WEIGHTED) ce_sum += nu * t; else ce_sum += t;
            }
        }
        float r[NPX], h[NPX];
        CE_PX r[c] = ok[c] ? gw / ce_at(se, c) : 0.f;
        CE_PX h[c] = ok[c] ? gw : 0.f;
        float* d = dlogits + b * K * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                CE_PX ce_at(g, c) = ce_at(v[k], c) * r[c] - (lab[c] == k ? h[c] : 0.f);
                if (live) ce_stpx<NPX>(d + k * HW, g);
                if constexpr (!__is_same(NT, ce_no_nhwc)) v[k] = g;
            }
        if constexpr (NPX == 1) ce_store_nhwc1<KMAX, NT>(v, K, dl_nhwc, dl_ldc, pix);
        else if constexpr (XCH) {
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
    ce_block_pair<false>(wave_sum(ce_sum), 0.f, partial);
}

// The class-incremental step (build-defined, parity unpinned: the reference has no continual-learning code; the definitions are the "MiB"
// losses of Cermelli et al., CVPR 2020, restated in include/clamd.h).  Classes [0, c_old) are old, [c_old, K) new, 0 is background:
//   unbiased CE   label y <  c_old: -(LSE(old) - LSE(all))          gradient  softmax_all - [k < c_old] softmax_old
//                 label y >= c_old: -(z_y - LSE(all))                          softmax_all - [k == y]            mean over the valid pixels
//   unbiased KD   q = softmax(zo[0 .. c_old)),  -(1 / c_old) (q_0 (LSE(bgnew) - LSE(all)) + sum_{1 <= k < c_old} q_k (z_k - LSE(all)))
//                 gradient softmax_all - [k in bgnew] q_0 exp(z_k - LSE(bgnew)) - [1 <= k < c_old] q_k          mean over ALL pixels, times lam
// ce4_kernel's shape: NPX = 4 consecutive pixels per thread, 16-byte accesses, e_k = exp(z_k - max) computed ONCE per logit and kept in
// the logit's register; sum_old e, sum_new e and e_0 give the three log-sum-exps.  KOLD > 0: the distillation term, exp(zo_k - max) of the
// c_old <= KOLD old-model logits kept in KOLD more registers per pixel (one exponential each; instantiated per (KMAX, KOLD) so that
// K = 21, c_old = 11 holds 24 + 16 float4).  A group whose largest logit lies 41 or more below the pixel's maximum (sum < 1e-18) has lost its
// exponentials to underflow: the rare `rebase` branch reloads that group's logits and takes them relative to the group's own maximum
// (fO / fN carry the shift), so  LSE(old) - LSE(all) and softmax_old stay exact however far apart the groups are.
// With c_old == 1 and KOLD == 0 every operation on the path to d logits and to the loss is the one ce4_kernel makes (bit-equal results).
// NPX = 1: the same arithmetic, one pixel per thread with 4-byte accesses, for H * W % 4 != 0 or unaligned tensors.
template <int KMAX, int KOLD, int NPX, typename NT>
__global__ void __launch_bounds__(256) ce4u_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                   const float* __restrict__ old_logits, int K_old_total, int c_old, float kd_scale,
                                                   float* __restrict__ dlogits, float* __restrict__ partial, int B, int K, long long HW,
                                                   long long ignore_index, float grad_scale, NT* dl_nhwc, int dl_ldc,
                                                   const unsigned int* __restrict__ count_rows) {
    constexpr bool KD = KOLD > 0;
    constexpr float NEG = -INFINITY, TINY = 1e-18f;
    __shared__ unsigned int cnt_tmp[4];
    const long long nq = (long long)B * HW / NPX;
    const unsigned int nv = ce_count_total(count_rows, 0, cnt_tmp);
    const float gs = grad_scale / (float)max(nv, 1u);
    const float gk = KD ? grad_scale * kd_scale : 0.f;             // kd_scale = lam / (c_old * B * H * W)
    float ce_sum = 0.f, kd_sum = 0.f;
    constexpr bool XCH = NPX == 4 && __is_same(NT, bf16_t) && CE_EXCHANGE;
    __shared__ uint4 xbuf[XCH ? 4 : 1][XCH ? 1024 : 1];
    for (long long base = (long long)blockIdx.x * blockDim.x; base < nq; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool live = i < nq;                                    // the trip count is block-uniform (the exchange has barriers)
        if (!XCH && !live) continue;
        const long long pix = NPX * (live ? i : nq - 1), b = pix / HW, p = pix - b * HW;
        const float* z = logits + b * K * HW + p;
        float4 v[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) v[k] = ce_ldpx<NPX>(z + k * HW);
        long long lab[4];
        ce_ld_labels<NPX>(labels, pix, lab);
        // ---- the old model: o[k] = exp(zo_k - max), rq = 1 / sum
        float4 o[KD ? KOLD : 1], rq = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (KD) {
            const float* zo = old_logits + b * K_old_total * HW + p;
            float4 mo = make_float4(NEG, NEG, NEG, NEG), so = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < KOLD; ++k)
                if (k < c_old) {
                    o[k] = ce_ldpx<NPX>(zo + k * HW);
                    CE_PX ce_at(mo, c) = fmaxf(ce_at(mo, c), ce_at(o[k], c));
                }
#pragma unroll
            for (int k = 0; k < KOLD; ++k)
                if (k < c_old) CE_PX { ce_at(o[k], c) = expf(ce_at(o[k], c) - ce_at(mo, c)); ce_at(so, c) += ce_at(o[k], c); }
            CE_PX ce_at(rq, c) = 1.f / ce_at(so, c);
        }
        // ---- the maxima of the two groups, then one exponential per logit
        float4 mO = make_float4(NEG, NEG, NEG, NEG), mN = mO, mx;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) CE_PX {
                ce_at(mO, c) = k < c_old ? fmaxf(ce_at(mO, c), ce_at(v[k], c)) : ce_at(mO, c);
                ce_at(mN, c) = k < c_old ? ce_at(mN, c) : fmaxf(ce_at(mN, c), ce_at(v[k], c));
            }
        CE_PX ce_at(mx, c) = fmaxf(ce_at(mO, c), ce_at(mN, c));
        const float4 z0 = v[0];
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f), sO = se, sN = se, vmO = se, picked = se, dot = se;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) CE_PX {
                float& e = ce_at(v[k], c);
                ce_at(picked, c) = lab[c] == k ? e : ce_at(picked, c);
                if constexpr (KD) { if (k >= 1 && k < KOLD) ce_at(dot, c) += k < c_old ? ce_at(o[k < KOLD ? k : 0], c) * (e - ce_at(mx, c)) : 0.f; }
                e = expf(e - ce_at(mx, c));
                ce_at(se, c) += e;                                   // in ce4_kernel's order
                ce_at(sO, c) = k < c_old ? ce_at(se, c) : ce_at(sO, c);       // the prefix sum at k = c_old - 1
                ce_at(vmO, c) = k < c_old ? fmaxf(ce_at(vmO, c), e) : ce_at(vmO, c);
                ce_at(sN, c) += k < c_old ? 0.f : e;
            }
        bool ok[NPX], yold[NPX];
        CE_PX { ok[c] = lab[c] != ignore_index && lab[c] >= 0 && lab[c] < K; yold[c] = ok[c] && lab[c] < c_old; }
        // ---- underflowed groups (rare): their exponentials again, relative to the group's own maximum
        float fO[NPX], fN[NPX], bN[NPX];
        CE_PX { fO[c] = fN[c] = 1.f; bN[c] = ce_at(mx, c); }
        bool nO[NPX], nN[NPX], anyO = false, anyN = false;
        CE_PX { nO[c] = yold[c] && ce_at(sO, c) < TINY; nN[c] = KD && c_old < K && ce_at(sN, c) < TINY; anyO |= nO[c]; anyN |= nN[c]; }
        if (anyO) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < c_old && k < K) {
                    const float4 t = ce_ldpx<NPX>(z + k * HW);
                    CE_PX { if (nO[c]) ce_at(v[k], c) = expf(ce_at(t, c) - ce_at(mO, c)); ce_at(s, c) += ce_at(v[k], c); }
                }
            CE_PX if (nO[c]) { ce_at(sO, c) = ce_at(s, c); ce_at(vmO, c) = 1.f; fO[c] = expf(ce_at(mO, c) - ce_at(mx, c)); }
        }
        if (anyN) {
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k >= c_old && k < K) {
                    const float4 t = ce_ldpx<NPX>(z + k * HW);
                    CE_PX { if (nN[c]) ce_at(v[k], c) = expf(ce_at(t, c) - ce_at(mN, c)); ce_at(s, c) += ce_at(v[k], c); }
                }
            CE_PX if (nN[c]) { ce_at(sN, c) = ce_at(s, c); bN[c] = ce_at(mN, c); fN[c] = expf(ce_at(mN, c) - ce_at(mx, c)); }
        }
        // ---- the loss terms and the per-pixel coefficients of the gradient
        float rAO[NPX], rAN[NPX], h[NPX], hO[NPX], den[NPX], kq[NPX] = {}, kb0[NPX] = {}, kbN[NPX] = {};
        CE_PX {
            const float lse = ce_at(mx, c) + logf(ce_at(se, c));
            if (live && ok[c])
                ce_sum += yold[c] ? lse - (ce_at(mO, c) + logf(ce_at(sO, c) / ce_at(vmO, c))) : lse - ce_at(picked, c);
            float rA = ok[c] ? gs / ce_at(se, c) : 0.f;
            h[c] = ok[c] ? gs : 0.f;
            hO[c] = yold[c] ? gs : 0.f;
            den[c] = yold[c] ? ce_at(sO, c) : 1.f;
            if constexpr (KD) {
                rA = ((ok[c] ? gs : 0.f) + gk) / ce_at(se, c);
                // LSE(bgnew) from z_0 and LSE(new) in the log domain: no second pass of exponentials, no underflow.  Both relative to bN, the
                // base of the new group's exponentials: bN + log(sum) would round LSE(new) to an ulp of |bN| (2^-17 at logits near 100), and
                // exp(z - LSE(bgnew)) would carry that as a relative error into the gradient of the background and of every new class
                const float lN = logf(ce_at(sN, c));                         // LSE(new) - bN; -inf when there is no new class
                const float z0r = ce_at(z0, c) - bN[c];
                const float hi = fmaxf(z0r, lN), lo = fminf(z0r, lN);
                const float lbg = hi + log1pf(expf(lo - hi));                // LSE(bgnew) - bN
                const float q0 = ce_at(o[0], c) * ce_at(rq, c);
                if (live) kd_sum -= q0 * (lbg + (bN[c] - ce_at(mx, c))) + ce_at(rq, c) * ce_at(dot, c) - logf(ce_at(se, c));
                kq[c] = gk * ce_at(rq, c);
                kb0[c] = gk * q0 * expf(z0r - lbg);
                kbN[c] = gk * q0 * expf(-lbg);
            }
            rAO[c] = rA * fO[c];
            rAN[c] = rA * fN[c];
        }
        float* d = dlogits + b * K * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                float4 g;
                if (k < c_old) {
                    CE_PX {
                        const float e = ce_at(v[k], c);
                        float t = fmaf(e, rAO[c], -((e / den[c]) * hO[c]));
                        if constexpr (KD) t -= k == 0 ? kb0[c] : ce_at(o[k < KOLD ? k : 0], c) * kq[c];
                        ce_at(g, c) = t;
                    }
                } else {
                    CE_PX {
                        const float e = ce_at(v[k], c);
                        float t = fmaf(e, rAN[c], -(lab[c] == k ? h[c] : 0.f));
                        if constexpr (KD) t -= e * kbN[c];
                        ce_at(g, c) = t;
                    }
                }
                if (live) ce_stpx<NPX>(d + k * HW, g);
                if constexpr (!__is_same(NT, ce_no_nhwc)) v[k] = g;
            }
        if constexpr (NPX == 4) ce_store_nhwc4<KMAX, NT, XCH>(v, K, dl_nhwc, dl_ldc, pix, base, nq, xbuf);
        else ce_store_nhwc1<KMAX, NT>(v, K, dl_nhwc, dl_ldc, pix);
    }
    ce_block_pair<true>(wave_sum(ce_sum), wave_sum(kd_sum), partial);
}

// out3 = {total, ce, kd} from the nblocks partial pairs (summed in double, in a fixed order); totals = {valid, bad} from the count rows
__global__ void ce_finalize_kernel(const float* __restrict__ partial, int nblocks, unsigned int* totals,
                                   float inv_npix, float lam, float* out3, const unsigned int* __restrict__ count_rows) {
    __shared__ unsigned int cnt_tmp[2][4];
    const unsigned int nvalid = ce_count_total(count_rows, 0, cnt_tmp[0]), nbad = ce_count_total(count_rows, 1, cnt_tmp[1]);
    if (threadIdx.x == 0) { totals[0] = nvalid; totals[1] = nbad; }
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    const ce_tree_row* red = ce_tree_pair(a, b);
    if (threadIdx.x == 0) {
        const float ce = (float)(red[0][0] / (double)max(nvalid, 1u));
        const float kd = (float)(red[1][0] * inv_npix * lam);
        out3[0] = ce + kd; out3[1] = ce; out3[2] = kd;
    }
}

// ---- class weights, label smoothing, focal term (clamd_ce_class_fwd_bwd; the definition is in include/clamd.h) ------------------------
// The family's shape with a per-class count in front: class_count_rows_kernel (one partial row {n_0 .. n_31, valid, bad} per workgroup) ->
// class_totals_kernel (one workgroup: the rows added, D = sum_k w_k n_k and W = sum_k w_k in fp64 in ascending k) -> ce4c_kernel (ce4_kernel's
// shape; a {nll, smo} partial pair per workgroup) -> cec_finalize_kernel.  Behind the CE workspace, in 32-bit words: the totals block
// {n_k[32], D (a double), W (a float), spare}, then the CE_COUNT_BLOCKS partial rows.
constexpr int CEC_KP = 32;
constexpr int CEC_ROW_WORDS = CEC_KP + 2, CEC_ROW_VALID = CEC_KP, CEC_ROW_BAD = CEC_KP + 1;
constexpr int CEC_TOT_D = CEC_KP, CEC_TOT_W = CEC_KP + 2, CEC_TOT_WORDS = CEC_KP + 4;
constexpr int CEC_WS_TOT = CE_WS_WORDS;
constexpr int CEC_WS_ROWS = CEC_WS_TOT + CEC_TOT_WORDS;
constexpr int CEC_WS_WORDS = CEC_WS_ROWS + CE_COUNT_BLOCKS * CEC_ROW_WORDS;
static_assert((CEC_WS_TOT + CEC_TOT_D) % 2 == 0, "D is a double: 8-byte aligned inside an 8-byte aligned workspace");

// The histogram of a workgroup's labels in LDS (integer atomics: any order, the same sums), left as one row with plain stores.  NPX = 4:
// 32-byte label loads (the pixel count a multiple of 4, the labels 32-byte aligned).
template <int NPX>
__global__ void __launch_bounds__(256) class_count_rows_kernel(const long long* __restrict__ labels, long long n, long long ignore_index, int K,
                                                               unsigned int* rows /* [CE_COUNT_BLOCKS][CEC_ROW_WORDS] */) {
    __shared__ unsigned int lh[CEC_KP + 1];                     // n_k, then the bad labels
    if (threadIdx.x <= CEC_KP) lh[threadIdx.x] = 0u;
    __syncthreads();
    const long long nq = n / NPX;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += (long long)gridDim.x * 256) {
        long long lab[4];
        ce_ld_labels<NPX>(labels, NPX * i, lab);
        CE_PX {
            const long long l = lab[c];
            if (l != ignore_index) atomicAdd(&lh[(l >= 0 && l < K) ? (int)l : CEC_KP], 1u);
        }
    }
    __syncthreads();
    unsigned int* row = rows + blockIdx.x * CEC_ROW_WORDS;
    if (threadIdx.x < CEC_KP) row[threadIdx.x] = lh[threadIdx.x];
    else if (threadIdx.x == CEC_KP) {
        unsigned int nv = 0;
        for (int k = 0; k < CEC_KP; ++k) nv += lh[k];
        row[CEC_ROW_VALID] = nv;
        row[CEC_ROW_BAD] = lh[CEC_KP];
    }
}

// One workgroup: thread (slice s = t / 34, column c = t % 34) adds rows s, s + 7, ... (integers); thread c < 34 adds the 7 slices.  Then D
// and W by one thread, in fp64, k ascending.  totals = {valid, bad} where loss._LossFn and the other criteria keep them.
constexpr int CEC_SLICES = 256 / CEC_ROW_WORDS;                 // 7
__global__ void __launch_bounds__(256) class_totals_kernel(const unsigned int* __restrict__ rows, const float* __restrict__ class_weight, int K,
                                                           unsigned int* totals, unsigned int* tot /* the totals block */) {
    __shared__ unsigned int part[CEC_SLICES][CEC_ROW_WORDS];
    __shared__ unsigned int col[CEC_ROW_WORDS];
    const int t = threadIdx.x, s = t / CEC_ROW_WORDS, c = t - s * CEC_ROW_WORDS;
    if (s < CEC_SLICES) {
        unsigned int a = 0;
        for (int r = s; r < CE_COUNT_BLOCKS; r += CEC_SLICES) a += rows[r * CEC_ROW_WORDS + c];
        part[s][c] = a;
    }
    __syncthreads();
    if (t < CEC_ROW_WORDS) {
        unsigned int a = 0;
        for (int j = 0; j < CEC_SLICES; ++j) a += part[j][t];
        col[t] = a;
        if (t < CEC_KP) tot[t] = a;
        else totals[t - CEC_KP] = a;
    }
    __syncthreads();
    if (t == 0) {
        double D = 0.0, Wd = 0.0;
        for (int k = 0; k < K; ++k) { D += (double)class_weight[k] * (double)col[k]; Wd += (double)class_weight[k]; }
        *reinterpret_cast<double*>(tot + CEC_TOT_D) = D;
        reinterpret_cast<float*>(tot)[CEC_TOT_W] = (float)Wd;
        tot[CEC_TOT_W + 1] = 0u;
    }
}

// ce4_kernel with the class weight of the pixel's label in its coefficient and, by MODE, one more term:
//   a = gs * nu_b * w_y (gs = grad_scale / (float)D; nu_b = 1.0f without image weights), d logits_k = e_k * (a' / se) - [k = y] a' with
//   CEC_WEIGHT   a' = a.  Every w_k == 1.0f: each operation is ce4_kernel's in ce4_kernel's order (the same bits, weighted or not)
//   CEC_SMOOTH   a' = a * (1 - eps), plus  e_k * (b W / se) - w_k b,  b = gs * nu_b * eps / K;  the second partial column is the sum of
//                nu_b * sum_k w_k (-log p_k) = nu_b * (sum_k w_k (max - z_k) + W log se): positive terms, no W * lse - sum w z cancellation
//   CEC_FOCAL    a' = a * f,  f = q^gamma (1 + gamma p_y t / q);  q = (sum_{k != y} e_k) / se, never 1 - p_y;  t = -log1p(-q) for q < 1/2 and
//                log se - (z_y - max) above (the difference first: t to an ulp of t, not of max);  t / q = 1 at q == 0
// w_k is wave-uniform: read with constant indices inside the unrolled class loops (scalar loads), w_y picked by picked's select chain.
enum { CEC_WEIGHT = 0, CEC_SMOOTH = 1, CEC_FOCAL = 2 };
template <int KMAX, int NPX, typename NT, int MODE>
__global__ void __launch_bounds__(256) ce4c_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                   const float* __restrict__ class_weight, const float* __restrict__ image_weight,
                                                   float* __restrict__ dlogits, float* __restrict__ partial, int B, int K, long long HW,
                                                   long long ignore_index, float grad_scale, float keep /* 1 - eps */, float spread /* eps / K */,
                                                   float gamma, NT* dl_nhwc, int dl_ldc, const float* __restrict__ tot) {
    const long long nq = (long long)B * HW / NPX;
    const double Dd = *reinterpret_cast<const double*>(tot + CEC_TOT_D);
    const float Wsum = tot[CEC_TOT_W];
    const float gs = Dd > 0.0 ? grad_scale / (float)Dd : 0.f;      // D == 0: every gradient exactly 0
    float ce_sum = 0.f, sm_sum = 0.f;
    constexpr bool XCH = NPX == 4 && __is_same(NT, bf16_t) && CE_EXCHANGE;
    __shared__ uint4 xbuf[XCH ? 4 : 1][XCH ? 1024 : 1];
    for (long long base = (long long)blockIdx.x * blockDim.x; base < nq; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool live = i < nq;                                    // the trip count is block-uniform (the exchange has barriers)
        if (!XCH && !live) continue;
        const long long pix = NPX * (live ? i : nq - 1), b = pix / HW, p = pix - b * HW;
        float nu = 1.f;
        if (image_weight) nu = image_weight[b];
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
        ce_ld_labels<NPX>(labels, pix, lab);
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f), picked = se, wy = se, ey = se, sq = se, swz = se;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                const float wk = class_weight[k];
                CE_PX ce_at(picked, c) = lab[c] == k ? ce_at(v[k], c) : ce_at(picked, c);
                CE_PX ce_at(wy, c) = lab[c] == k ? wk : ce_at(wy, c);
                if constexpr (MODE == CEC_SMOOTH) CE_PX ce_at(swz, c) = fmaf(wk, ce_at(mx, c) - ce_at(v[k], c), ce_at(swz, c));
                CE_PX ce_at(v[k], c) = expf(ce_at(v[k], c) - ce_at(mx, c));
                CE_PX ce_at(se, c) += ce_at(v[k], c);
                if constexpr (MODE == CEC_FOCAL) CE_PX {
                    ce_at(ey, c) = lab[c] == k ? ce_at(v[k], c) : ce_at(ey, c);
                    ce_at(sq, c) += lab[c] == k ? 0.f : ce_at(v[k], c);
                }
            }
        bool ok[NPX];
        CE_PX ok[c] = lab[c] != ignore_index && lab[c] >= 0 && lab[c] < K;
        float r[NPX], h[NPX], rs[NPX], hs[NPX];
        CE_PX {
            const float wn = nu * ce_at(wy, c);
            float a = gw * ce_at(wy, c);                             // the pixel's coefficient gs * nu_b * w_y
            if constexpr (MODE == CEC_FOCAL) {
                const float q = ce_at(sq, c) / ce_at(se, c), py = ce_at(ey, c) / ce_at(se, c);
                const float t = q < 0.5f ? -log1pf(-q) : logf(ce_at(se, c)) - (ce_at(picked, c) - ce_at(mx, c));
                const float qg = powf(q, gamma);
                a *= qg * fmaf(gamma * py, q > 0.f ? t / q : 1.f, 1.f);
                if (live && ok[c]) ce_sum += wn * (qg * t);
            } else {
                if (live && ok[c]) {
                    const float t = ce_at(mx, c) + logf(ce_at(se, c)) - ce_at(picked, c);
                    ce_sum += wn * t;
                }
            }
            if constexpr (MODE == CEC_SMOOTH) {
                a *= keep;
                if (live && ok[c]) sm_sum += nu * fmaf(Wsum, logf(ce_at(se, c)), ce_at(swz, c));
                const float bsm = gw * spread;
                rs[c] = ok[c] ? bsm * Wsum / ce_at(se, c) : 0.f;
                hs[c] = ok[c] ? bsm : 0.f;
            }
            r[c] = ok[c] ? a / ce_at(se, c) : 0.f;
            h[c] = ok[c] ? a : 0.f;
        }
        float* d = dlogits + b * K * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                CE_PX ce_at(g, c) = ce_at(v[k], c) * r[c] - (lab[c] == k ? h[c] : 0.f);
                if constexpr (MODE == CEC_SMOOTH) {
                    const float wk = class_weight[k];
                    CE_PX ce_at(g, c) += fmaf(ce_at(v[k], c), rs[c], -(wk * hs[c]));
                }
                if (live) ce_stpx<NPX>(d + k * HW, g);
                if constexpr (!__is_same(NT, ce_no_nhwc)) v[k] = g;
            }
        if constexpr (NPX == 4) ce_store_nhwc4<KMAX, NT, XCH>(v, K, dl_nhwc, dl_ldc, pix, base, nq, xbuf);
        else ce_store_nhwc1<KMAX, NT>(v, K, dl_nhwc, dl_ldc, pix);
    }
    ce_sum = wave_sum(ce_sum);
    if constexpr (MODE == CEC_SMOOTH) sm_sum = wave_sum(sm_sum);
    ce_block_pair<true>(ce_sum, sm_sum, partial);      // two columns in every mode: the LDS of the kernel as it was (four zeros add to 0.f)
}

// out3 = {loss, keep * nll / D, spread * smo / D} from the nblocks partial pairs, ce_finalize_kernel's fixed-order fp64 sums; D == 0: zeros
__global__ void __launch_bounds__(256) cec_finalize_kernel(const float* __restrict__ partial, int nblocks, const float* __restrict__ tot,
                                                           double keep, double spread, float* out3) {
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { a += partial[2 * i]; b += partial[2 * i + 1]; }
    const ce_tree_row* red = ce_tree_pair(a, b);
    if (threadIdx.x == 0) {
        const double D = *reinterpret_cast<const double*>(tot + CEC_TOT_D);
        const float nll = D > 0.0 ? (float)(keep * (red[0][0] / D)) : 0.f;
        const float smo = D > 0.0 ? (float)(spread * (red[1][0] / D)) : 0.f;
        out3[0] = nll + smo; out3[1] = nll; out3[2] = smo;
    }
}

// ---- cross-entropy + soft Dice (build-defined; the definitions are restated in include/clamd.h) --------------------------------------
// Dice is not per-pixel: its gradient at a pixel depends on the per-class sums I = sum p_k [y = k], P = sum p_k, Y = sum [y = k] over the
// pixel's group (the batch, or its image).  Three passes, every reduction in a fixed order:
//   dice_sums_kernel   logits + labels once, ce4_kernel's access shape; a workgroup owns a chunk of ONE image and leaves one partial row
//   dice_coef_kernel   one workgroup per group: the rows added in fp64, then N, D, |S|, the pair {c, a} per class and the group's loss term
//   dice_grad_kernel   logits + labels again: softmax recomputed, d logits (NCHW and optionally NHWC), one CE partial pair per workgroup
//   dice_finalize_kernel
// A partial row, in 32-bit words: I[32], P[32] (fp32), Y[32] (unsigned), {bad, valid, -, -}.
constexpr int DICE_KP = 32;
constexpr int DICE_ROW_WORDS = 3 * DICE_KP + 4;
constexpr int DICE_ROW_BAD = 3 * DICE_KP, DICE_ROW_VALID = 3 * DICE_KP + 1;
constexpr int DICE_MAX_ROWS = CE_MAX_BLOCKS;                   // workgroups of the two per-pixel passes = partial rows = CE partial pairs

// a[i] summed over the 64 lanes, N = 16, 32 or 64 values per lane: halving exchanges (lane bit 32 decides who keeps which half of the
// values, then bit 16, ...) -- N - 1 shuffles instead of 6 N -- then a butterfly over the lane bits that are left.  Afterwards a[0] of lane l
// is the total of value l >> (6 - log2 N).  A fixed tree: the same bits every run.
template <int N, int H = N / 2, int BIT = 32>
__device__ inline void dice_wave_reduce(float (&a)[N], int lane) {
    if constexpr (H >= 1) {
        const bool up = lane & BIT;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const float keep = up ? a[j + H] : a[j], send = up ? a[j] : a[j + H];
            a[j] = keep + __shfl_xor(send, BIT);
        }
        dice_wave_reduce<N, H / 2, BIT / 2>(a, lane);
    } else if constexpr (BIT >= 1) {
        a[0] += __shfl_xor(a[0], BIT);
        dice_wave_reduce<N, 0, BIT / 2>(a, lane);
    }
}

// KP2: KMAX rounded up to a power of two (the reduction's width); workgroup blockIdx.x = image * cpi + chunk
template <int KMAX, int NPX>
__global__ void __launch_bounds__(256) dice_sums_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                        float* __restrict__ rows, int cpi, int K, long long HW, long long ignore_index) {
    PASS_PRIO();
    constexpr int KP2 = KMAX == 24 ? 32 : KMAX, N = 2 * KP2, SHIFT = N == 64 ? 0 : N == 32 ? 1 : 2;
    __shared__ float red[4][N];
    __shared__ unsigned int cnt[DICE_KP + 1];                   // Y_k, then the bad labels: integer atomics in LDS (any order, same sum)
    const int b = blockIdx.x / cpi, chunk = blockIdx.x - b * cpi;
    if (threadIdx.x <= DICE_KP) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long long nq = HW / NPX;
    const float* zb = logits + (long long)b * K * HW;
    const long long* lb = labels + (long long)b * HW;
    float acc[N];                                               // [0, KP2): I_k   [KP2, 2 KP2): P_k
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    for (long long i = (long long)chunk * 256 + threadIdx.x; i < nq; i += (long long)cpi * 256) {
        const long long p = NPX * i;
        const float* z = zb + p;
        float4 v[KMAX];
        float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                v[k] = ce_ldpx<NPX>(z + k * HW);
                CE_PX ce_at(mx, c) = fmaxf(ce_at(mx, c), ce_at(v[k], c));
            }
        long long lab[4];
        ce_ld_labels<NPX>(lb, p, lab);
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                CE_PX ce_at(v[k], c) = expf(ce_at(v[k], c) - ce_at(mx, c));
                CE_PX ce_at(se, c) += ce_at(v[k], c);
            }
        float r[NPX];
        CE_PX {
            const bool ok = lab[c] != ignore_index && lab[c] >= 0 && lab[c] < K;
            r[c] = ok ? 1.f / ce_at(se, c) : 0.f;                // an invalid pixel adds zeros
            if (ok) atomicAdd(&cnt[(int)lab[c]], 1u);
            else if (lab[c] != ignore_index) atomicAdd(&cnt[DICE_KP], 1u);
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) CE_PX {
                const float pk = ce_at(v[k], c) * r[c];
                acc[KP2 + k] += pk;
                acc[k] += lab[c] == k ? pk : 0.f;
            }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    dice_wave_reduce<N>(acc, lane);
    if ((lane & ((1 << SHIFT) - 1)) == 0) red[wv][lane >> SHIFT] = acc[0];
    __syncthreads();
    float* row = rows + (long long)blockIdx.x * DICE_ROW_WORDS;
    const int t = threadIdx.x;
    if (t < N) {
        const int k = t < KP2 ? t : t - KP2;
        if (k < K) row[(t < KP2 ? 0 : DICE_KP) + k] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    } else if (t >= 64 && t < 64 + DICE_KP) {
        reinterpret_cast<unsigned int*>(row)[t] = cnt[t - 64];          // word 64 + k: Y_k
    } else if (t == 128) {
        unsigned int nv = 0;
        for (int k = 0; k < DICE_KP; ++k) nv += cnt[k];
        reinterpret_cast<unsigned int*>(row)[DICE_ROW_BAD] = cnt[DICE_KP];
        reinterpret_cast<unsigned int*>(row)[DICE_ROW_VALID] = nv;
    }
}

// One workgroup of 512 threads per group g: rows [g * rows_per_group, (g + 1) * rows_per_group).  Thread (slice s = t / 32, class k = t % 32)
// adds rows s, s + 16, ... in fp64, eight rows' loads in flight per trip; the 16 slices are added in order.  coef[g][k] = {c_gk, a_gk} (zero
// outside S_g), gterm[g] = the group's loss term 1 - mean dice (0 for an empty S_g).  Workgroup 0 also totals {valid, bad} over ALL rows into
// totals[0 .. 1].  (Slices, loads in flight and the times they gave: DESIGN.md, the kernel table's Dice row.)
constexpr int DICE_SLICES = 16;
__global__ void __launch_bounds__(32 * DICE_SLICES) dice_coef_kernel(const float* __restrict__ rows, int nrows, int rows_per_group, int G, int K,
                                                        double w_dice, double smooth, int first_class, int present_only,
                                                        float* __restrict__ coef, double* __restrict__ gterm, unsigned int* __restrict__ totals) {
    SIDE_PRIO();
    __shared__ double sI[DICE_SLICES][DICE_KP], sP[DICE_SLICES][DICE_KP], sdice[DICE_KP];
    __shared__ unsigned long long sY[DICE_SLICES][DICE_KP];
    __shared__ unsigned int wtot[2][DICE_SLICES / 2];
    const int t = threadIdx.x, k = t & 31, s = t >> 5, g = blockIdx.x;
    // eight rows per trip, every load of a trip issued before its first add (a row past the end is read from row r and adds zeros)
    double aI = 0.0, aP = 0.0;
    unsigned long long aY = 0;
    const int r1 = (g + 1) * rows_per_group;
    if (k < K)
        for (int r = g * rows_per_group + s; r < r1; r += 8 * DICE_SLICES) {
            float vi[8], vp[8];
            unsigned int vy[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int rr = r + j * DICE_SLICES;
                const float* row = rows + (long long)(rr < r1 ? rr : r) * DICE_ROW_WORDS;
                vi[j] = row[k]; vp[j] = row[DICE_KP + k]; vy[j] = reinterpret_cast<const unsigned int*>(row)[2 * DICE_KP + k];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool in = r + j * DICE_SLICES < r1;
                aI += in ? (double)vi[j] : 0.0; aP += in ? (double)vp[j] : 0.0; aY += in ? vy[j] : 0u;
            }
        }
    if (g == 0) {                                                // the label totals: per wave by shuffles, the waves added below
        unsigned int nv = 0, nb = 0;
        for (int r = t; r < nrows; r += 32 * DICE_SLICES) {
            const unsigned int* row = reinterpret_cast<const unsigned int*>(rows) + (long long)r * DICE_ROW_WORDS;
            nb += row[DICE_ROW_BAD]; nv += row[DICE_ROW_VALID];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o); nb += __shfl_xor(nb, o); }
        if ((t & 63) == 0) { wtot[0][t >> 6] = nv; wtot[1][t >> 6] = nb; }
    }
    sI[s][k] = aI; sP[s][k] = aP; sY[s][k] = aY;
    __syncthreads();
    if (g == 0 && t < 2) {
        unsigned int n = 0;
        for (int j = 0; j < DICE_SLICES / 2; ++j) n += wtot[t][j];
        totals[t] = n;
    }
    int nS = 0;
    if (t < DICE_KP) {                                           // the first half of wave 0: class k = t
        double I = 0.0, P = 0.0;
        unsigned long long Y = 0;
        for (int j = 0; j < DICE_SLICES; ++j) { I += sI[j][k]; P += sP[j][k]; Y += sY[j][k]; }
        const bool in_set = k >= first_class && k < K && (!present_only || Y > 0);
        nS = __popcll(__ballot(in_set));
        const double u = nS ? w_dice / ((double)G * (double)nS) : 0.0;
        const double Nk = 2.0 * I + smooth, Dk = P + (double)Y + smooth;
        const bool flat = !in_set || Dk == 0.0;                 // D == 0: dice = 1 and no gradient
        sdice[k] = in_set ? (Dk == 0.0 ? 1.0 : Nk / Dk) : 0.0;
        coef[((long long)g * DICE_KP + k) * 2 + 0] = flat ? 0.f : (float)(u * Nk / (Dk * Dk));
        coef[((long long)g * DICE_KP + k) * 2 + 1] = flat ? 0.f : (float)(-2.0 * u / Dk);
    }
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int j = 0; j < DICE_KP; ++j) sum += sdice[j];
        gterm[g] = nS ? 1.0 - sum / (double)nS : 0.0;
    }
}

// ce4_kernel's shape and arithmetic for the cross-entropy part (gce = grad_scale * w_ce / max(N, 1)); the Dice part from the group's table:
// g_k = c_k + [y = k] a_y, dot = sum_k p_k g_k = (sum_k e_k c_k) / se + p_y a_y,
//   d logits_k = e_k * (gce / se + (grad_scale / se) * (g_k - dot)) - [y = k] gce          on a valid pixel, 0 elsewhere.
// c_k is workgroup-uniform (a workgroup stays inside one image): scalar registers; a_y is looked up by the label: LDS.
template <int KMAX, int NPX, typename NT>
__global__ void __launch_bounds__(256) dice_grad_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                        const float* __restrict__ coef, const unsigned int* __restrict__ totals,
                                                        float* __restrict__ dlogits, float* __restrict__ partial, int cpi, int per_image,
                                                        int K, long long HW, long long ignore_index, float grad_scale, float w_ce,
                                                        NT* dl_nhwc, int dl_ldc) {
    PASS_PRIO();
    __shared__ float ta[DICE_KP];
    constexpr bool XCH = NPX == 4 && __is_same(NT, bf16_t) && CE_EXCHANGE;
    __shared__ uint4 xbuf[XCH ? 4 : 1][XCH ? 1024 : 1];
    const int b = blockIdx.x / cpi, chunk = blockIdx.x - b * cpi;
    const float* cf = coef + (long long)(per_image ? b : 0) * (2 * DICE_KP);
    if (threadIdx.x < DICE_KP) ta[threadIdx.x] = cf[2 * threadIdx.x + 1];
    float ck[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) ck[k] = cf[2 * k];
    __syncthreads();
    const float gce = grad_scale * w_ce / (float)max(totals[0], 1u);
    const long long nq = HW / NPX, q0 = (long long)b * nq;       // quads (pixels) of an image; the image's first
    float ce_sum = 0.f;
    for (long long lbase = (long long)chunk * 256; lbase < nq; lbase += (long long)cpi * 256) {
        const long long i = lbase + threadIdx.x;
        const bool live = i < nq;                                    // the trip count is block-uniform (the exchange has barriers)
        if (!XCH && !live) continue;
        const long long p = NPX * (live ? i : nq - 1), pix = (long long)b * HW + p;
        const float* z = logits + (long long)b * K * HW + p;
        float4 v[KMAX];
        float4 mx = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                v[k] = ce_ldpx<NPX>(z + k * HW);
                CE_PX ce_at(mx, c) = fmaxf(ce_at(mx, c), ce_at(v[k], c));
            }
        long long lab[4];
        ce_ld_labels<NPX>(labels, pix, lab);
        float4 se = make_float4(0.f, 0.f, 0.f, 0.f), picked = se, ey = se, dc = se;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                CE_PX ce_at(picked, c) = lab[c] == k ? ce_at(v[k], c) : ce_at(picked, c);
                CE_PX ce_at(v[k], c) = expf(ce_at(v[k], c) - ce_at(mx, c));
                CE_PX ce_at(se, c) += ce_at(v[k], c);
                CE_PX ce_at(ey, c) = lab[c] == k ? ce_at(v[k], c) : ce_at(ey, c);
                CE_PX ce_at(dc, c) = fmaf(ce_at(v[k], c), ck[k], ce_at(dc, c));
            }
        float rce[NPX], rd[NPX], h[NPX], ay[NPX], dot[NPX];
        CE_PX {
            const bool ok = lab[c] != ignore_index && lab[c] >= 0 && lab[c] < K;
            if (live && ok) ce_sum += ce_at(mx, c) + logf(ce_at(se, c)) - ce_at(picked, c);
            const float rinv = 1.f / ce_at(se, c);
            ay[c] = ta[ok ? (int)lab[c] : 0];
            ay[c] = ok ? ay[c] : 0.f;
            dot[c] = fmaf(ce_at(ey, c) * rinv, ay[c], ce_at(dc, c) * rinv);
            rce[c] = ok ? gce * rinv : 0.f;
            rd[c] = ok ? grad_scale * rinv : 0.f;
            h[c] = ok ? gce : 0.f;
        }
        float* d = dlogits + (long long)b * K * HW + p;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
                CE_PX {
                    const bool hit = lab[c] == k;
                    const float gk = ck[k] + (hit ? ay[c] : 0.f);
                    ce_at(g, c) = ce_at(v[k], c) * fmaf(rd[c], gk - dot[c], rce[c]) - (hit ? h[c] : 0.f);
                }
                if (live) ce_stpx<NPX>(d + k * HW, g);
                if constexpr (!__is_same(NT, ce_no_nhwc)) v[k] = g;
            }
        // the NHWC copy: `base` and the bound are this image's -- the exchange must not reach into the next image from the tail's dead lanes
        if constexpr (NPX == 4) ce_store_nhwc4<KMAX, NT, XCH>(v, K, dl_nhwc, dl_ldc, pix, q0 + lbase, q0 + nq, xbuf);
        else ce_store_nhwc1<KMAX, NT>(v, K, dl_nhwc, dl_ldc, pix);
    }
    ce_block_pair<false>(wave_sum(ce_sum), 0.f, partial);
}

// loss3 = {ce + dice, ce = w_ce * mean CE, dice = w_dice * mean_g gterm}: the CE partials and the group terms added in fp64 in a fixed order
__global__ void __launch_bounds__(256) dice_finalize_kernel(const float* __restrict__ partial, int nblocks, const unsigned int* __restrict__ totals,
                                                            const double* __restrict__ gterm, int G, double w_ce, double w_dice, float* out3) {
    double a = 0, b = 0;
    for (int i = threadIdx.x; i < nblocks; i += 256) a += partial[2 * i];
    for (int i = threadIdx.x; i < G; i += 256) b += gterm[i];
    const ce_tree_row* red = ce_tree_pair(a, b);
    if (threadIdx.x == 0) {
        const float ce = (float)(w_ce * (red[0][0] / (double)max(totals[0], 1u)));
        const float dice = (float)(w_dice * (red[1][0] / (double)G));
        out3[0] = ce + dice; out3[1] = ce; out3[2] = dice;
    }
}

}  // namespace clamd

using namespace clamd;

// ------------------------------------------------------------------------------------------------ host side
// What the entry points share: the argument checks, whether the four-pixel form applies, the grid, the pieces of the workspace.
struct CePlan {
    long long HW, npix;
    bool four;               // H * W % 4 == 0 and every per-pixel tensor aligned for 16-byte (labels: 32-byte) accesses
    int grid;                // workgroups of the loss kernel = partial pairs the finalize adds
    float* partial;
    unsigned int *totals, *rows;
    hipStream_t s;
};

static int ce_fail(const char* who, const char* text) {
    static thread_local char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", who, text);
    return clamd_fail(msg);
}

// `who` prefixes the messages; `old_logits` may be null; dl_nhwc null: no NHWC copy; four_ok: the caller has a four-pixel kernel for this call
static int ce_plan(CePlan* p, const char* who, bool four_ok, const float* logits, const long long* labels, const float* old_logits, const float* dlogits,
                   const void* dl_nhwc, int dl_ldc, int dl_dtype, const float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H,
                   int W, void* stream) {
    if (!logits || !labels || !dlogits || !loss3 || !workspace || B <= 0 || H <= 0 || W <= 0) return ce_fail(who, "null pointer or empty shape");
    if (K < 1 || K > 32) return ce_fail(who, "number of classes must be in [1, 32]");
    if (ws_bytes < clamd_ce_workspace_bytes()) return clamd_fail("ce: workspace too small");
    if (((size_t)logits % 4) || ((size_t)dlogits % 4) || ((size_t)old_logits % 4) || ((size_t)labels % 8)) return ce_fail(who, "misaligned tensor");
    if (dl_nhwc) {
        if (dl_ldc < 32 || dl_ldc % 8 || ((size_t)dl_nhwc % 16)) return ce_fail(who, "the NHWC copy needs a pitch >= 32 channels, a multiple of 8, and a 16-byte aligned base");
        if (dl_dtype != CLAMD_BF16 && dl_dtype != CLAMD_F32 && dl_dtype != CLAMD_SPLIT) return ce_fail(who, "bad dtype");
        if (int e = clamd_check_split(dl_dtype, dl_nhwc, dl_ldc)) return e;
    }
    p->HW = (long long)H * W;
    p->npix = B * p->HW;
    p->four = four_ok && p->HW % 4 == 0 && ((size_t)logits % 16) == 0 && ((size_t)dlogits % 16) == 0 && ((size_t)old_logits % 16) == 0 && ((size_t)labels % 32) == 0;
    const long long g = ((p->four ? p->npix / 4 : p->npix) + 255) / 256;
    p->grid = g > CE_MAX_BLOCKS ? CE_MAX_BLOCKS : (int)g;
    p->partial = (float*)workspace;
    p->totals = (unsigned int*)workspace + CE_WS_TOTALS;
    p->rows = (unsigned int*)workspace + CE_WS_ROWS;
    p->s = (hipStream_t)stream;
    return 0;
}

// The family's one dispatch: f(nt, kmax, npx) with the element type of the NHWC copy (ce_plan has checked dl_dtype; dl_nhwc null: ce_no_nhwc)
// and the kernel's shape: (32, 1), one pixel per thread, when !p.four; else (KMAX, 4), KMAX the smallest multiple of 8 that holds K.
// CE_T / CE_V: a tag's type / value inside f.
template <typename T> struct ce_type { using type = T; };
template <int N> using ce_int = std::integral_constant<int, N>;
#define CE_T(tag) typename decltype(tag)::type
#define CE_V(tag) decltype(tag)::value
template <typename F> static void ce_dispatch(const CePlan& p, int K, const void* dl_nhwc, int dl_dtype, F f) {
    auto shaped = [&](auto nt) {
        if (!p.four) f(nt, ce_int<32>{}, ce_int<1>{});
        else if (K <= 8) f(nt, ce_int<8>{}, ce_int<4>{});
        else if (K <= 16) f(nt, ce_int<16>{}, ce_int<4>{});
        else if (K <= 24) f(nt, ce_int<24>{}, ce_int<4>{});
        else f(nt, ce_int<32>{}, ce_int<4>{});
    };
    if (!dl_nhwc) shaped(ce_type<ce_no_nhwc>{});
    else if (dl_dtype == CLAMD_BF16) shaped(ce_type<bf16_t>{});
    else if (dl_dtype == CLAMD_F32) shaped(ce_type<float>{});
    else shaped(ce_type<split_t>{});
}

// ce4_kernel, plain (WT = ce_no_weight; four pixels only: the callers have no other use) or weighted (WT = const float*)
template <typename WT>
static void ce_launch(const CePlan& p, const float* logits, const long long* labels, WT weight, float* dlogits, void* dl_nhwc, int dl_ldc,
                      int dl_dtype, int B, int K, long long ignore_index, float grad_scale) {
    constexpr bool WEIGHTED = !__is_same(WT, ce_no_weight);
    ce_dispatch(p, K, dl_nhwc, dl_dtype, [&](auto nt, auto kmax, auto npx) {
        if constexpr (WEIGHTED || CE_V(npx) == 4)
            hipLaunchKernelGGL((ce4_kernel<CE_V(kmax), CE_V(npx), CE_T(nt), WEIGHTED>), dim3(p.grid), dim3(256), 0, p.s, logits, labels, weight,
                               dlogits, p.partial, B, K, p.HW, ignore_index, grad_scale, (CE_T(nt)*)dl_nhwc, dl_ldc, p.rows);
    });
}

// lam: the factor of the kd partial sums' mean over all pixels
static void ce_finalize(const CePlan& p, float lam, float* loss3) {
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, p.s, p.partial, p.grid, p.totals, (float)(1.0 / (double)p.npix), lam, loss3, p.rows);
}

static void ce_count(const long long* labels, long long npix, long long ignore_index, int K, unsigned int* rows, hipStream_t s) {
    hipLaunchKernelGGL(count_valid_rows_kernel, dim3(CE_COUNT_BLOCKS), dim3(256), 0, s, labels, npix, ignore_index, K, rows);
}

// The grid of the two per-pixel Dice passes and the pieces of their workspace behind the CE workspace.  A workgroup owns a chunk of one image:
// cpi chunks per image, as many as 256-lane trips cover it, capped so that B * cpi <= DICE_MAX_ROWS (a capped workgroup loops).  The
// offsets are those of the one-pixel form (the larger row count), so the layout does not depend on the alignment of a call's tensors.
struct DicePlan {
    int cpi, nrows, G;       // chunks per image, partial rows = workgroups, groups
    long long rows, coef, gterm, words;      // offsets and size in 32-bit words
};
static bool dice_plan(DicePlan* d, int B, int K, int H, int W, int per_image, bool four) {
    if (B <= 0 || H <= 0 || W <= 0 || K < 1 || K > 32 || B > DICE_MAX_ROWS) return false;
    const long long HW = (long long)H * W, cap = DICE_MAX_ROWS / B;
    const long long want1 = (HW + 255) / 256, want = ((four ? HW / 4 : HW) + 255) / 256;
    d->cpi = (int)(want < cap ? want : cap);
    d->nrows = B * d->cpi;
    d->G = per_image ? B : 1;
    d->rows = CE_WS_WORDS;
    d->coef = d->rows + (long long)B * (want1 < cap ? want1 : cap) * DICE_ROW_WORDS;
    d->gterm = d->coef + (long long)d->G * 2 * DICE_KP;
    d->words = d->gterm + 2LL * d->G;
    return true;
}

extern "C" {

size_t clamd_ce_dice_workspace_bytes(int B, int K, int H, int W, int per_image) {
    DicePlan d;
    return dice_plan(&d, B, K, H, W, per_image, false) ? (size_t)d.words * 4 : 0;
}

int clamd_ce_dice_fwd_bwd(const float* logits, const long long* labels, float* dlogits, void* dl_nhwc, int dl_ldc, int dl_dtype,
                          float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W, long long ignore_index,
                          double w_ce, double w_dice, double smooth, int first_class, int present_only, int per_image,
                          double grad_scale, void* stream) {
    const char* who = "ce_dice";
    if (first_class != 0 && first_class != 1) return ce_fail(who, "first_class must be 0 or 1");
    if (!(w_ce >= 0.0) || !(w_dice >= 0.0) || !(smooth >= 0.0) || !isfinite(w_ce) || !isfinite(w_dice) || !isfinite(smooth))
        return ce_fail(who, "w_ce, w_dice and smooth must be finite and >= 0");
    if (workspace && ws_bytes < clamd_ce_workspace_bytes()) return ce_fail(who, "workspace too small (clamd_ce_dice_workspace_bytes)");
    CePlan p;
    if (int e = ce_plan(&p, who, true, logits, labels, nullptr, dlogits, dl_nhwc, dl_ldc, dl_dtype, loss3, workspace, ws_bytes, B, K, H, W, stream)) return e;
    DicePlan d;
    if (!dice_plan(&d, B, K, H, W, per_image, p.four)) return ce_fail(who, "more than 2048 images: every image needs a partial row of its own and the coefficient pass adds at most 2048");
    if (ws_bytes < (size_t)d.words * 4) return ce_fail(who, "workspace too small (clamd_ce_dice_workspace_bytes)");
    if ((size_t)workspace % 16) return ce_fail(who, "workspace must be 16-byte aligned");
    float* ws = (float*)workspace;
    float *rows = ws + d.rows, *coef = ws + d.coef;
    double* gterm = (double*)(ws + d.gterm);
    const float gs = (float)grad_scale;
    ce_dispatch(p, K, nullptr, 0, [&](auto, auto kmax, auto npx) {            // the sums pass writes no copy: no element type
        hipLaunchKernelGGL((dice_sums_kernel<CE_V(kmax), CE_V(npx)>), dim3(d.nrows), dim3(256), 0, p.s, logits, labels, rows, d.cpi, K, p.HW,
                           ignore_index);
    });
    hipLaunchKernelGGL(dice_coef_kernel, dim3(d.G), dim3(32 * DICE_SLICES), 0, p.s, rows, d.nrows, per_image ? d.cpi : d.nrows, d.G, K, w_dice, smooth,
                       first_class, present_only ? 1 : 0, coef, gterm, p.totals);
    ce_dispatch(p, K, dl_nhwc, dl_dtype, [&](auto nt, auto kmax, auto npx) {
        using NT = CE_T(nt);
        hipLaunchKernelGGL((dice_grad_kernel<CE_V(kmax), CE_V(npx), NT>), dim3(d.nrows), dim3(256), 0, p.s, logits, labels, coef, p.totals, dlogits,
                           p.partial, d.cpi, per_image ? 1 : 0, K, p.HW, ignore_index, gs, (float)w_ce, (NT*)dl_nhwc, dl_ldc);
    });
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, p.s, p.partial, d.nrows, p.totals, gterm, d.G, w_ce, w_dice, loss3);
    return clamd_check_launch("ce_dice_fwd_bwd");
}

size_t clamd_ce_workspace_bytes(void) { return (size_t)CE_WS_WORDS * 4; }
size_t clamd_ce_bad_label_count_offset(void) { return (size_t)(CE_WS_TOTALS + 1) * 4; }

int clamd_ce_fwd_bwd(const float* logits, const long long* labels, const float* old_logits, int K_old_total, int c_old,
                     double temperature, double lam, float* dlogits, float* loss3, void* workspace, size_t ws_bytes,
                     int B, int K, int H, int W, long long ignore_index, double grad_scale, void* stream) {
    CePlan p;
    if (int e = ce_plan(&p, "ce", !old_logits, logits, labels, old_logits, dlogits, nullptr, 0, 0, loss3, workspace, ws_bytes, B, K, H, W, stream)) return e;
    if (old_logits && (c_old < 1 || c_old > K || c_old > K_old_total)) return clamd_fail("ce: bad c_old");
    ce_count(labels, p.npix, ignore_index, K, p.rows, p.s);
    if (p.four)
        ce_launch(p, logits, labels, ce_no_weight{}, dlogits, nullptr, 0, 0, B, K, ignore_index, (float)grad_scale);
    else      // the distillation term, odd sizes, misaligned storage: one pixel per thread
        hipLaunchKernelGGL(ce_kernel<32>, dim3(p.grid), dim3(256), 0, p.s, logits, labels, old_logits, K_old_total, c_old,
                           (float)(1.0 / temperature), (float)lam, dlogits, p.partial, p.rows, B, K, p.HW, ignore_index, (float)grad_scale);
    ce_finalize(p, (float)lam, loss3);
    return clamd_check_launch("ce_fwd_bwd");
}

int clamd_ce_count(const long long* labels, int B, int K, int H, int W, long long ignore_index, void* workspace, size_t ws_bytes, void* stream) {
    if (K < 1 || K > 32 || !labels || B <= 0 || H <= 0 || W <= 0) return clamd_fail("ce_count: bad arguments");
    if (ws_bytes < clamd_ce_workspace_bytes()) return clamd_fail("ce: workspace too small");
    ce_count(labels, (long long)B * H * W, ignore_index, K, (unsigned int*)workspace + CE_WS_ROWS, (hipStream_t)stream);
    return clamd_check_launch("ce_count");
}

int clamd_ce_fwd_bwd_counted(const float* logits, const long long* labels, float* dlogits, void* dl_nhwc, int dl_ldc, int dl_dtype,
                             float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W, long long ignore_index,
                             double grad_scale, void* stream) {
    CePlan p;
    if (int e = ce_plan(&p, "ce_fwd_bwd_counted", true, logits, labels, nullptr, dlogits, dl_nhwc, dl_ldc, dl_dtype, loss3, workspace, ws_bytes, B, K, H, W, stream)) return e;
    if (!p.four) return clamd_fail("ce_fwd_bwd_counted: needs H * W % 4 == 0 and 16-byte aligned logits / 32-byte aligned labels (use clamd_ce_fwd_bwd)");
    ce_launch(p, logits, labels, ce_no_weight{}, dlogits, dl_nhwc, dl_ldc, dl_dtype, B, K, ignore_index, (float)grad_scale);
    ce_finalize(p, 0.f, loss3);
    return clamd_check_launch("ce_fwd_bwd_counted");
}

int clamd_ce_fwd_bwd_weighted(const float* logits, const long long* labels, const float* image_weight, float* dlogits, void* dl_nhwc,
                              int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W,
                              long long ignore_index, double grad_scale, void* stream) {
    if (!image_weight || ((size_t)image_weight % 4)) return clamd_fail("ce_weighted: image_weight (B floats) is required (clamd_ce_fwd_bwd_counted is the unweighted loss)");
    CePlan p;
    if (int e = ce_plan(&p, "ce_weighted", true, logits, labels, nullptr, dlogits, dl_nhwc, dl_ldc, dl_dtype, loss3, workspace, ws_bytes, B, K, H, W, stream)) return e;
    ce_launch(p, logits, labels, image_weight, dlogits, dl_nhwc, dl_ldc, dl_dtype, B, K, ignore_index, (float)grad_scale);
    ce_finalize(p, 0.f, loss3);
    return clamd_check_launch("ce_fwd_bwd_weighted");
}

int clamd_ce_unbiased_fwd_bwd(const float* logits, const long long* labels, const float* old_logits, int K_old_total, int c_old, double lam,
                              float* dlogits, void* dl_nhwc, int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes,
                              int B, int K, int H, int W, long long ignore_index, double grad_scale, void* stream) {
    if (c_old < 1 || c_old > K) return clamd_fail("ce_unbiased: c_old must be in [1, K]");
    if (!(lam >= 0.0)) return clamd_fail("ce_unbiased: lam must be >= 0");
    if (lam == 0.0) old_logits = nullptr;
    if (old_logits && c_old > K_old_total) return clamd_fail("ce_unbiased: c_old exceeds the old model's class count K_old_total");
    CePlan p;
    if (int e = ce_plan(&p, "ce_unbiased", true, logits, labels, old_logits, dlogits, dl_nhwc, dl_ldc, dl_dtype, loss3, workspace, ws_bytes, B, K, H, W, stream)) return e;
    const float kd_scale = old_logits ? (float)(lam / ((double)c_old * (double)p.npix)) : 0.f;
    // ce4u_kernel<KMAX, KOLD, NPX, NT>: KOLD in {0, 16, 32} sizes the register array of the old model's exponentials (only its first c_old
    // entries are touched); the odd-size path is not tuned: one instantiation per term
    const int ko = !old_logits ? 0 : c_old <= 16 ? 16 : 32;
    ce_dispatch(p, K, dl_nhwc, dl_dtype, [&](auto nt, auto kmax, auto npx) {
        using NT = CE_T(nt);
        auto launch = [&](auto kold) {
            hipLaunchKernelGGL((ce4u_kernel<CE_V(kmax), CE_V(kold), CE_V(npx), NT>), dim3(p.grid), dim3(256), 0, p.s, logits, labels, old_logits,
                               K_old_total, c_old, kd_scale, dlogits, p.partial, B, K, p.HW, ignore_index, (float)grad_scale, (NT*)dl_nhwc, dl_ldc,
                               p.rows);
        };
        if (ko == 0) launch(ce_int<0>{});
        else if constexpr (CE_V(npx) == 1) launch(ce_int<32>{});
        else if (ko == 16) launch(ce_int<16>{});
        else if constexpr (CE_V(kmax) > 16) launch(ce_int<32>{});      // c_old > 16 needs K > 16
    });
    // the kernel leaves sum_px of c_old * kd_px: the finalize multiplies by 1 / npix and by its `lam` argument
    ce_finalize(p, old_logits ? (float)(lam / (double)c_old) : 0.f, loss3);
    return clamd_check_launch("ce_unbiased_fwd_bwd");
}

size_t clamd_ce_class_workspace_bytes(void) { return (size_t)CEC_WS_WORDS * 4; }

int clamd_ce_class_fwd_bwd(const float* logits, const long long* labels, const float* class_weight, const float* image_weight, float* dlogits,
                           void* dl_nhwc, int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W,
                           long long ignore_index, double label_smoothing, double focal_gamma, double grad_scale, void* stream) {
    const char* who = "ce_class";
    if (!class_weight || ((size_t)class_weight % 4)) return ce_fail(who, "class_weight (K floats) is required and must be 4-byte aligned");
    if ((size_t)image_weight % 4) return ce_fail(who, "misaligned image_weight");
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0)) return ce_fail(who, "label_smoothing must be in [0, 1)");
    if (!(focal_gamma >= 0.0) || !isfinite(focal_gamma)) return ce_fail(who, "focal_gamma must be finite and >= 0");
    if (label_smoothing > 0.0 && focal_gamma > 0.0) return ce_fail(who, "label_smoothing and focal_gamma are both non-zero: the combination is not defined");
    if (workspace && (ws_bytes < clamd_ce_class_workspace_bytes() || ((size_t)workspace % 8)))
        return ce_fail(who, "workspace too small (clamd_ce_class_workspace_bytes) or not 8-byte aligned");
    CePlan p;
    if (int e = ce_plan(&p, who, true, logits, labels, nullptr, dlogits, dl_nhwc, dl_ldc, dl_dtype, loss3, workspace, ws_bytes, B, K, H, W, stream)) return e;
    unsigned int* tot = (unsigned int*)workspace + CEC_WS_TOT;
    unsigned int* crows = (unsigned int*)workspace + CEC_WS_ROWS;
    if (p.npix % 4 == 0 && ((size_t)labels % 32) == 0)
        hipLaunchKernelGGL(class_count_rows_kernel<4>, dim3(CE_COUNT_BLOCKS), dim3(256), 0, p.s, labels, p.npix, ignore_index, K, crows);
    else
        hipLaunchKernelGGL(class_count_rows_kernel<1>, dim3(CE_COUNT_BLOCKS), dim3(256), 0, p.s, labels, p.npix, ignore_index, K, crows);
    hipLaunchKernelGGL(class_totals_kernel, dim3(1), dim3(256), 0, p.s, crows, class_weight, K, p.totals, tot);
    const double keep = 1.0 - label_smoothing, spread = label_smoothing / (double)K;
    ce_dispatch(p, K, dl_nhwc, dl_dtype, [&](auto nt, auto kmax, auto npx) {
        using NT = CE_T(nt);
        auto launch = [&](auto mode) {
            hipLaunchKernelGGL((ce4c_kernel<CE_V(kmax), CE_V(npx), NT, CE_V(mode)>), dim3(p.grid), dim3(256), 0, p.s, logits, labels, class_weight,
                               image_weight, dlogits, p.partial, B, K, p.HW, ignore_index, (float)grad_scale, (float)keep, (float)spread,
                               (float)focal_gamma, (NT*)dl_nhwc, dl_ldc, (const float*)tot);
        };
        if (focal_gamma > 0.0) launch(ce_int<CEC_FOCAL>{});
        else if (label_smoothing > 0.0) launch(ce_int<CEC_SMOOTH>{});
        else launch(ce_int<CEC_WEIGHT>{});
    });
    hipLaunchKernelGGL(cec_finalize_kernel, dim3(1), dim3(256), 0, p.s, p.partial, p.grid, (const float*)tot, keep, spread, loss3);
    return clamd_check_launch("ce_class_fwd_bwd");
}

}  // extern "C"
