// Fused multi-tensor SGD with momentum, Nesterov and weight decay (+ the two build-defined pulls towards an anchor that the Adam kernels
// of misc.hip carry: L2-to-old-weights and elastic weight consolidation).  torch.optim.SGD semantics with dampening 0, maximize off:
//   g  = grad * grad_scale
//   g += (weight_decay * decay_mult) * p
//   d  = p - old;  g += 2 * l2_lambda * d;  g += ewc_lambda * omega * d          (anchor / importance only)
//   buf = mu * buf + g                                                            (momentum buffer only; a zero buffer gives buf = g)
//   u  = nesterov ? g + mu * buf : (buf ? buf : g)
//   p  = p - lr * u
// hyper (device, fp32[8]): [0] lr  [1] mu  [2] weight_decay  [3] nesterov  [4] grad_scale  [5] l2_lambda  [6] ewc_lambda  [7] 0
//
// HBM-bound: 20 B / parameter with momentum (p, g, buf read; p, buf written), +4 B with an anchor, +4 B with importance, 12 B without
// momentum.  One workgroup per (tensor, chunk) job as in the Adam step.  16-byte accesses: a chunk is shifted by the tensor's `head`
// (elements up to p's first 16-byte boundary, peeled by chunk 0), so every store to p is aligned; g, buf, old and omega may sit at any
// element phase (the engine packs gradients tightly) and go through a 4-byte-aligned vector type, as importance_accum_kernel does.  The
// last, partial group of a tensor goes element-wise.  A thread issues the loads of all its four groups before the first store, so up to
// 20 16-byte loads per lane are in flight.  Nothing outside [0, n) of any tensor is read or written.
#include "common.hip.h"
#include "clamd_internal.h"

namespace clamd {

struct SgdTensor { float* p; const float* g; float* buf; const float* old; long long n; float decay_mult; float pad; };
static_assert(sizeof(SgdTensor) == 48, "the host side builds 48-byte rows");
typedef float sgd_f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct SgdHyper { float lr, mu, wd, gs, l2x2, lam; bool nesterov; };

template <bool BUF, bool OLD, bool OM>
__device__ __forceinline__ float sgd_element(float p, float grad, float& buf, float old, float om, const SgdHyper& h, float& l2sum,
                                             float& esum) {
    float g = grad * h.gs;
    g += h.wd * p;
    if (OLD) {
        const float d = p - old;
        g += h.l2x2 * d;
        l2sum += d * d;
        if (OM) {
            g += h.lam * om * d;
            esum += om * (d * d);
        }
    }
    float u = g;
    if (BUF) {
        buf = h.mu * buf + g;
        u = h.nesterov ? g + h.mu * buf : buf;
    }
    return p - h.lr * u;
}

template <bool BUF, bool OLD, bool OM>
__device__ __forceinline__ void sgd_chunk(const SgdTensor& t, const float* __restrict__ om, int chunk, const SgdHyper& h, float& l2sum,
                                          float& esum) {
    constexpr int GROUPS = ADAM_CHUNK / 1024;
    const int head = (int)((4u - (unsigned)(((size_t)t.p >> 2) & 3u)) & 3u);
    auto one = [&](long long i) {
        float b = BUF ? t.buf[i] : 0.f;
        t.p[i] = sgd_element<BUF, OLD, OM>(t.p[i], t.g[i], b, OLD ? t.old[i] : 0.f, OM ? om[i] : 0.f, h, l2sum, esum);
        if (BUF) t.buf[i] = b;
    };
    if (chunk == 0 && (int)threadIdx.x < head && (long long)threadIdx.x < t.n) one(threadIdx.x);
    const long long base = (long long)chunk * ADAM_CHUNK + head;
    float4 p[GROUPS];
    sgd_f32x4_a4 g[GROUPS], b[GROUPS], o[GROUPS], w[GROUPS];
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        const long long i = base + 4 * (k * 256 + (int)threadIdx.x);
        if (i + 4 <= t.n) {
            p[k] = *(const float4*)(t.p + i);
            g[k] = *(const sgd_f32x4_a4*)(t.g + i);
            if (BUF) b[k] = *(const sgd_f32x4_a4*)(t.buf + i);
            if (OLD) o[k] = *(const sgd_f32x4_a4*)(t.old + i);
            if (OM) w[k] = *(const sgd_f32x4_a4*)(om + i);
        }
    }
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        const long long i = base + 4 * (k * 256 + (int)threadIdx.x);
        if (i + 4 <= t.n) {
            float4 q;
            float b0 = BUF ? b[k].x : 0.f, b1 = BUF ? b[k].y : 0.f, b2 = BUF ? b[k].z : 0.f, b3 = BUF ? b[k].w : 0.f;
            q.x = sgd_element<BUF, OLD, OM>(p[k].x, g[k].x, b0, OLD ? o[k].x : 0.f, OM ? w[k].x : 0.f, h, l2sum, esum);
            q.y = sgd_element<BUF, OLD, OM>(p[k].y, g[k].y, b1, OLD ? o[k].y : 0.f, OM ? w[k].y : 0.f, h, l2sum, esum);
            q.z = sgd_element<BUF, OLD, OM>(p[k].z, g[k].z, b2, OLD ? o[k].z : 0.f, OM ? w[k].z : 0.f, h, l2sum, esum);
            q.w = sgd_element<BUF, OLD, OM>(p[k].w, g[k].w, b3, OLD ? o[k].w : 0.f, OM ? w[k].w : 0.f, h, l2sum, esum);
            *(float4*)(t.p + i) = q;
            if (BUF) *(sgd_f32x4_a4*)(t.buf + i) = sgd_f32x4_a4{b0, b1, b2, b3};
        } else {
            for (long long j = i; j < t.n; ++j) one(j);
        }
    }
}

// EWC: an importance table was given.  A row without an anchor takes neither pull, whatever the table says.
template <bool EWC>
__global__ void __launch_bounds__(256) sgd_kernel(const SgdTensor* __restrict__ tensors, const float* const* __restrict__ importance,
                                                  const AdamChunk* __restrict__ chunks, const float* __restrict__ hyper,
                                                  float* ewc_accum, float* l2_accum) {
    const AdamChunk c = chunks[blockIdx.x];
    SgdTensor t = tensors[c.tensor];
    SgdHyper h;
    h.lr = hyper[0]; h.mu = hyper[1]; h.wd = hyper[2] * t.decay_mult; h.nesterov = hyper[3] != 0.f;
    h.gs = hyper[4]; h.l2x2 = 2.f * hyper[5]; h.lam = hyper[6];
    float l2sum = 0.f, esum = 0.f;
    if (EWC && t.old) {
        const float* om = importance[c.tensor];
        if (t.buf) sgd_chunk<true, true, true>(t, om, c.chunk, h, l2sum, esum);
        else sgd_chunk<false, true, true>(t, om, c.chunk, h, l2sum, esum);
    } else if (t.old) {
        if (t.buf) sgd_chunk<true, true, false>(t, nullptr, c.chunk, h, l2sum, esum);
        else sgd_chunk<false, true, false>(t, nullptr, c.chunk, h, l2sum, esum);
    } else {
        if (t.buf) sgd_chunk<true, false, false>(t, nullptr, c.chunk, h, l2sum, esum);
        else sgd_chunk<false, false, false>(t, nullptr, c.chunk, h, l2sum, esum);
    }
    if (EWC || l2_accum) {
        // as adam_kernel: no float atomics, one partial per workgroup (shuffle tree, then the four waves in a fixed order)
        __shared__ float wsum[2][4];
        esum = wave_sum(esum);
        l2sum = wave_sum(l2sum);
        if ((threadIdx.x & 63) == 0) { wsum[0][threadIdx.x >> 6] = esum; wsum[1][threadIdx.x >> 6] = l2sum; }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (EWC) ewc_accum[1 + blockIdx.x] = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
            if (l2_accum) l2_accum[1 + blockIdx.x] = (wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3]);
        }
    }
}

}  // namespace clamd

using namespace clamd;

extern "C" {

int clamd_sizeof_sgd_tensor(void) { return (int)sizeof(SgdTensor); }

int clamd_sgd_step(const void* tensors_dev, const void* importance_dev, const void* chunks_dev, int nchunks, const float* hyper_dev,
                   float* ewc_accum_dev, float* l2_accum_dev, void* stream) {
    if (nchunks <= 0) return clamd_fail("sgd_step: no chunks");
    if (!tensors_dev || !chunks_dev) return clamd_fail("sgd_step: null tensor or chunk table");
    if (!hyper_dev) return clamd_fail("sgd_step: null hyper buffer");
    if (importance_dev && !ewc_accum_dev) return clamd_fail("sgd_step: an importance table needs a penalty buffer (1 + nchunks floats)");
    if (!importance_dev && ewc_accum_dev) return clamd_fail("sgd_step: a consolidation penalty buffer without an importance table");
    hipStream_t s = (hipStream_t)stream;
    if (importance_dev) {
        hipLaunchKernelGGL(sgd_kernel<true>, dim3(nchunks), dim3(256), 0, s, (const SgdTensor*)tensors_dev,
                           (const float* const*)importance_dev, (const AdamChunk*)chunks_dev, hyper_dev, ewc_accum_dev, l2_accum_dev);
        clamd_launch_partial_sum(ewc_accum_dev, nchunks, s);
    } else {
        hipLaunchKernelGGL(sgd_kernel<false>, dim3(nchunks), dim3(256), 0, s, (const SgdTensor*)tensors_dev,
                           (const float* const*)nullptr, (const AdamChunk*)chunks_dev, hyper_dev, (float*)nullptr, l2_accum_dev);
    }
    if (l2_accum_dev) clamd_launch_partial_sum(l2_accum_dev, nchunks, s);
    return clamd_check_launch("sgd_step");
}

}  // extern "C"
