// The multi-tensor passes: fused Adam (plain and with elastic weight consolidation), fused SGD, both with or without the path integral of
// Synaptic Intelligence, the importance accumulation, the path integral's task boundary and the gradient norm of clipping.  All
// walk one job list of (tensor, ADAM_CHUNK-element chunk), one 256-thread workgroup per job, over a device table of per-tensor rows; they
// share the job list, the pull towards an anchor, the fixed-order penalty sums and the host-side checks below.
//
// Adam: torch.optim.Adam semantics (trainer.py:108-110,176): weight decay 0, amsgrad off, maximize off.
//   m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// hyper (device, fp32[8]): [0] lr  [1] beta1  [2] beta2  [3] eps  [4] grad_scale  [5] l2_lambda  [6] ewc_lambda
// state (device): step counter (int), derived[0] = lr/bc1, derived[1] = sqrt(bc2)
// 28 B / parameter (p, g, m, v read; p, m, v written), 36 B with an anchor and importance.
//
// SGD: torch.optim.SGD semantics with dampening 0, maximize off:
//   g  = grad * grad_scale
//   g += (weight_decay * decay_mult) * p
//   d  = p - old;  g += 2 * l2_lambda * d;  g += ewc_lambda * omega * d          (anchor / importance only)
//   buf = mu * buf + g                                                            (momentum buffer only; a zero buffer gives buf = g)
//   u  = nesterov ? g + mu * buf : (buf ? buf : g)
//   p  = p - lr * u
// hyper (device, fp32[8]): [0] lr  [1] mu  [2] weight_decay  [3] nesterov  [4] grad_scale  [5] l2_lambda  [6] ewc_lambda  [7] 0
// HBM-bound: 20 B / parameter with momentum (p, g, buf read; p, buf written), +4 B with an anchor, +4 B with importance, 12 B without
// momentum.
//
// Path integral (Synaptic Intelligence, Zenke et al. 2017; build-defined): the TRACK instantiations of both steps also do
//   omega += -(grad * grad_scale) * (p_new - p_old)
// with the gradient as it was handed over (before weight decay and the pulls) and the fp32 values read and stored: +8 B / parameter.  At a
// task boundary path_importance_kernel turns it into importance = decay * importance + max(0, omega) / ((p - start)^2 + xi), 20 B / element.
//
// SGD and the two importance passes use 16-byte accesses: a chunk is shifted by the tensor's `head` (elements up to the written tensor's first
// 16-byte boundary, peeled by chunk 0), so every vector store is aligned; the tensors that are only read may sit at any element phase (the
// engine packs gradients tightly) and go through a 4-byte-aligned vector type (gfx9 global memory takes dword-aligned wide accesses).  The
// last, partial group of a tensor goes element-wise.  Nothing outside [0, n) of any tensor is read or written.
#include <stdio.h>
#include "common.hip.h"
#include "clamd_internal.h"

namespace clamd {

struct AdamChunk { int tensor; int chunk; };
constexpr int ADAM_CHUNK = 4096;      // clamd_adam_chunk_elems()
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// elements of a tensor in front of its first 16-byte boundary
__device__ __forceinline__ int chunk_head(const void* p) { return (int)((4u - (unsigned)(((size_t)p >> 2) & 3u)) & 3u); }

// The two build-defined pulls towards an anchor, added to the gradient, and their penalty sums: the uniform
// L2-to-old-weights term and, with OM, the importance-weighted one of elastic weight consolidation.
template <bool OM>
__device__ __forceinline__ void anchor_pull(float p, float old, float om, float l2x2, float lam, float& g, float& l2sum, float& esum) {
    const float d = p - old;
    g += l2x2 * d;
    l2sum += d * d;
    if (OM) {
        g += lam * om * d;
        esum += om * (d * d);
    }
}

// The scaled gradient once more, for the path integral, from a copy of the raw gradient that the compiler cannot see through: the step's
// own grad * scale gains no second use, so its expressions contract as they do in the untracked instantiation and tracking leaves the
// step's results as they are.
__device__ __forceinline__ float task_gradient(float grad, float gs) {
    asm volatile("" : "+v"(grad));
    return grad * gs;
}

// out[j][1 + block] = this workgroup's sum of v[j], for every non-null out[j].  No float atomics: one partial per workgroup (shuffle tree,
// then the four waves in a fixed order); adam_l2_final_kernel adds the partials in a fixed order, so the reported penalty is
// bit-reproducible.
template <int N>
__device__ __forceinline__ void block_sums(const float (&v)[N], float* const (&out)[N]) {
    __shared__ float wsum[N][4];
    float s[N];
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = wave_sum(v[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) wsum[j][threadIdx.x >> 6] = s[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (out[j]) out[j][1 + blockIdx.x] = (wsum[j][0] + wsum[j][1]) + (wsum[j][2] + wsum[j][3]);
    }
}

// accum[0] = sum of the per-workgroup partials accum[1 .. n] in a fixed order (fp64): thread t adds partials t, t + 256, ...; then a
// fixed tree over the 256 threads
__global__ void __launch_bounds__(256) adam_l2_final_kernel(float* l2, int n) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)l2[1 + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) l2[0] = (float)red[0];
}

// ------------------------------------------------------------------------------------------------ Adam
struct AdamTensor { float* p; const float* g; float* m; float* v; const float* old; long long n; };
struct AdamHyper { float b2, eps, gs, l2x2, lam, step_size, bc2s, w1, w2; };

__global__ void adam_prepare_kernel(const float* hyper, int* step, float* derived) {
    const int s = *step + 1;
    *step = s;
    const double b1 = hyper[1], b2 = hyper[2];
    derived[0] = (float)((double)hyper[0] / (1.0 - pow(b1, (double)s)));
    derived[1] = (float)sqrt(1.0 - pow(b2, (double)s));
}

// Element i of one tensor.  EWC: the row has an anchor and `om` its importance; otherwise the anchor is optional and pulls uniformly.
// TRACK: `path` is the row's path integral, which takes -(the scaled gradient) * (the stored value - the value read).
template <bool EWC, bool TRACK>
__device__ __forceinline__ void adam_element(const AdamTensor& t, const float* __restrict__ om, float* __restrict__ path, long long i,
                                             const AdamHyper& h, float& l2sum, float& esum) {
    const float grad = t.g[i];
    float g = grad * h.gs;
    const float p = t.p[i];
    if (EWC) anchor_pull<true>(p, t.old[i], om[i], h.l2x2, h.lam, g, l2sum, esum);
    else if (t.old) anchor_pull<false>(p, t.old[i], 0.f, h.l2x2, h.lam, g, l2sum, esum);
    float m = t.m[i], v = t.v[i];
    // torch lerp: weight < 0.5 ? m + w*(g-m) : g - (g-m)*(1-w)
    m = (h.w1 < 0.5f) ? m + h.w1 * (g - m) : g - (g - m) * (1.f - h.w1);
    v = v * h.b2 + (h.w2 * g) * g;
    const float denom = sqrtf(v) / h.bc2s + h.eps;
    const float pn = p - h.step_size * (m / denom);
    t.p[i] = pn;
    t.m[i] = m; t.v[i] = v;
    if (TRACK) path[i] = path[i] - task_gradient(grad, h.gs) * (pn - p);
}

// EWC = false, TRACK = false is what every step without consolidation and tracking launches (importance, path and ewc_accum null).
// EWC = true: ewc_accum[1 + block] = this workgroup's sum omega d^2; either way l2_accum[1 + block] (optional) = its sum d^2.
template <bool EWC, bool TRACK>
__global__ void __launch_bounds__(256) adam_kernel(const AdamTensor* __restrict__ tensors, const float* const* __restrict__ importance,
                                                   float* const* __restrict__ paths, const AdamChunk* __restrict__ chunks,
                                                   const float* __restrict__ hyper, const float* __restrict__ derived, float* ewc_accum,
                                                   float* l2_accum) {
    const AdamChunk c = chunks[blockIdx.x];
    const AdamTensor t = tensors[c.tensor];
    const float* __restrict__ om = EWC ? importance[c.tensor] : nullptr;
    float* __restrict__ path = TRACK ? paths[c.tensor] : nullptr;
    const float b1 = hyper[1], b2 = hyper[2];
    const AdamHyper h = {b2, hyper[3], hyper[4], 2.f * hyper[5], EWC ? hyper[6] : 0.f, derived[0], derived[1], 1.f - b1, 1.f - b2};
    const long long base = (long long)c.chunk * ADAM_CHUNK;
    float l2sum = 0.f, esum = 0.f;
#pragma unroll 4
    for (int k = 0; k < ADAM_CHUNK / 256; ++k) {
        const long long i = base + k * 256 + threadIdx.x;
        if (i < t.n) adam_element<EWC, TRACK>(t, om, path, i, h, l2sum, esum);
    }
    if (EWC) block_sums<2>({esum, l2sum}, {ewc_accum, l2_accum});
    else if (l2_accum) block_sums<1>({l2sum}, {l2_accum});
}

// ------------------------------------------------------------------------------------------------ SGD
struct SgdTensor { float* p; const float* g; float* buf; const float* old; long long n; float decay_mult; float pad; };
static_assert(sizeof(SgdTensor) == 48, "the host side builds 48-byte rows");

struct SgdHyper { float lr, mu, wd, gs, l2x2, lam; bool nesterov; };

template <bool BUF, bool OLD, bool OM>
__device__ __forceinline__ float sgd_element(float p, float grad, float& buf, float old, float om, const SgdHyper& h, float& l2sum,
                                             float& esum) {
    float g = grad * h.gs;
    g += h.wd * p;
    if (OLD) anchor_pull<OM>(p, old, om, h.l2x2, h.lam, g, l2sum, esum);
    float u = g;
    if (BUF) {
        buf = h.mu * buf + g;
        u = h.nesterov ? g + h.mu * buf : buf;
    }
    return p - h.lr * u;
}

// A thread issues the loads of all its four groups before the first store, so up to 24 16-byte loads per lane are in flight.
// TRACK: `pa` is the row's path integral; it takes -(grad * grad_scale) * (the stored value - the value read), outside sgd_element.
template <bool BUF, bool OLD, bool OM, bool TRACK>
__device__ __forceinline__ void sgd_chunk(const SgdTensor& t, const float* __restrict__ om, float* __restrict__ pa, int chunk,
                                          const SgdHyper& h, float& l2sum, float& esum) {
    constexpr int GROUPS = ADAM_CHUNK / 1024;
    const int head = chunk_head(t.p);
    auto one = [&](long long i) {
        float b = BUF ? t.buf[i] : 0.f;
        const float p0 = t.p[i], gr = t.g[i];
        const float p1 = sgd_element<BUF, OLD, OM>(p0, gr, b, OLD ? t.old[i] : 0.f, OM ? om[i] : 0.f, h, l2sum, esum);
        t.p[i] = p1;
        if (BUF) t.buf[i] = b;
        if (TRACK) pa[i] = pa[i] - task_gradient(gr, h.gs) * (p1 - p0);
    };
    if (chunk == 0 && (int)threadIdx.x < head && (long long)threadIdx.x < t.n) one(threadIdx.x);
    const long long base = (long long)chunk * ADAM_CHUNK + head;
    float4 p[GROUPS];
    f32x4_a4 g[GROUPS], b[GROUPS], o[GROUPS], w[GROUPS], a[GROUPS];
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        const long long i = base + 4 * (k * 256 + (int)threadIdx.x);
        if (i + 4 <= t.n) {
            p[k] = *(const float4*)(t.p + i);
            g[k] = *(const f32x4_a4*)(t.g + i);
            if (BUF) b[k] = *(const f32x4_a4*)(t.buf + i);
            if (OLD) o[k] = *(const f32x4_a4*)(t.old + i);
            if (OM) w[k] = *(const f32x4_a4*)(om + i);
            if (TRACK) a[k] = *(const f32x4_a4*)(pa + i);
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
            if (BUF) *(f32x4_a4*)(t.buf + i) = f32x4_a4{b0, b1, b2, b3};
            if (TRACK)
                *(f32x4_a4*)(pa + i) = f32x4_a4{a[k].x - task_gradient(g[k].x, h.gs) * (q.x - p[k].x),
                                                a[k].y - task_gradient(g[k].y, h.gs) * (q.y - p[k].y),
                                                a[k].z - task_gradient(g[k].z, h.gs) * (q.z - p[k].z),
                                                a[k].w - task_gradient(g[k].w, h.gs) * (q.w - p[k].w)};
        } else {
            for (long long j = i; j < t.n; ++j) one(j);
        }
    }
}

// EWC: an importance table was given.  A row without an anchor takes neither pull, whatever the table says.  TRACK: a path table was given.
template <bool EWC, bool TRACK>
__global__ void __launch_bounds__(256) sgd_kernel(const SgdTensor* __restrict__ tensors, const float* const* __restrict__ importance,
                                                  float* const* __restrict__ paths, const AdamChunk* __restrict__ chunks,
                                                  const float* __restrict__ hyper, float* ewc_accum, float* l2_accum) {
    const AdamChunk c = chunks[blockIdx.x];
    SgdTensor t = tensors[c.tensor];
    SgdHyper h;
    h.lr = hyper[0]; h.mu = hyper[1]; h.wd = hyper[2] * t.decay_mult; h.nesterov = hyper[3] != 0.f;
    h.gs = hyper[4]; h.l2x2 = 2.f * hyper[5]; h.lam = hyper[6];
    float l2sum = 0.f, esum = 0.f;
    float* pa = TRACK ? paths[c.tensor] : nullptr;
    if (EWC && t.old) {
        const float* om = importance[c.tensor];
        if (t.buf) sgd_chunk<true, true, true, TRACK>(t, om, pa, c.chunk, h, l2sum, esum);
        else sgd_chunk<false, true, true, TRACK>(t, om, pa, c.chunk, h, l2sum, esum);
    } else if (t.old) {
        if (t.buf) sgd_chunk<true, true, false, TRACK>(t, nullptr, pa, c.chunk, h, l2sum, esum);
        else sgd_chunk<false, true, false, TRACK>(t, nullptr, pa, c.chunk, h, l2sum, esum);
    } else {
        if (t.buf) sgd_chunk<true, false, false, TRACK>(t, nullptr, pa, c.chunk, h, l2sum, esum);
        else sgd_chunk<false, false, false, TRACK>(t, nullptr, pa, c.chunk, h, l2sum, esum);
    }
    if (EWC || l2_accum) block_sums<2>({esum, l2sum}, {EWC ? ewc_accum : nullptr, l2_accum});
}

// ------------------------------------------------------------------------------------------------ importance
// dst = decay * dst + scale * (SQUARE ? src * src : src) over every tensor of a table.  12 B / element.
struct ImportanceTensor { float* dst; const float* src; long long n; };

template <bool SQUARE>
__global__ void __launch_bounds__(256) importance_accum_kernel(const ImportanceTensor* __restrict__ tensors,
                                                               const AdamChunk* __restrict__ chunks, float decay, float scale) {
    const AdamChunk c = chunks[blockIdx.x];
    const ImportanceTensor t = tensors[c.tensor];
    const int head = chunk_head(t.dst);
    auto one = [&](long long i) {
        const float s = t.src[i];
        t.dst[i] = decay * t.dst[i] + scale * (SQUARE ? s * s : s);
    };
    if (c.chunk == 0 && (int)threadIdx.x < head && (long long)threadIdx.x < t.n) one(threadIdx.x);
    const long long base = (long long)c.chunk * ADAM_CHUNK + head;
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 1024; ++k) {
        const long long i = base + 4 * (k * 256 + (int)threadIdx.x);
        if (i + 4 <= t.n) {
            const f32x4_a4 s = *(const f32x4_a4*)(t.src + i);
            float4 d = *(const float4*)(t.dst + i);
            d.x = decay * d.x + scale * (SQUARE ? s.x * s.x : s.x);
            d.y = decay * d.y + scale * (SQUARE ? s.y * s.y : s.y);
            d.z = decay * d.z + scale * (SQUARE ? s.z * s.z : s.z);
            d.w = decay * d.w + scale * (SQUARE ? s.w * s.w : s.w);
            *(float4*)(t.dst + i) = d;
        } else {
            for (long long j = i; j < t.n; ++j) one(j);
        }
    }
}

// The task boundary of the path integral: importance = decay * importance + max(0, path) / ((p - start)^2 + xi).  path, p and start are
// only read.  20 B / element.
struct PathTensor { float* importance; const float* path; const float* p; const float* start; long long n; };
static_assert(sizeof(PathTensor) == 40, "the host side builds 40-byte rows");

__device__ __forceinline__ float path_importance(float imp, float path, float p, float start, float decay, float xi) {
    const float d = p - start;
    return decay * imp + fmaxf(path, 0.f) / (d * d + xi);
}

__global__ void __launch_bounds__(256) path_importance_kernel(const PathTensor* __restrict__ tensors, const AdamChunk* __restrict__ chunks,
                                                              float decay, float xi) {
    const AdamChunk c = chunks[blockIdx.x];
    const PathTensor t = tensors[c.tensor];
    const int head = chunk_head(t.importance);
    auto one = [&](long long i) { t.importance[i] = path_importance(t.importance[i], t.path[i], t.p[i], t.start[i], decay, xi); };
    if (c.chunk == 0 && (int)threadIdx.x < head && (long long)threadIdx.x < t.n) one(threadIdx.x);
    const long long base = (long long)c.chunk * ADAM_CHUNK + head;
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / 1024; ++k) {
        const long long i = base + 4 * (k * 256 + (int)threadIdx.x);
        if (i + 4 <= t.n) {
            const f32x4_a4 a = *(const f32x4_a4*)(t.path + i), p = *(const f32x4_a4*)(t.p + i), s = *(const f32x4_a4*)(t.start + i);
            float4 w = *(const float4*)(t.importance + i);
            w.x = path_importance(w.x, a.x, p.x, s.x, decay, xi);
            w.y = path_importance(w.y, a.y, p.y, s.y, decay, xi);
            w.z = path_importance(w.z, a.z, p.z, s.z, decay, xi);
            w.w = path_importance(w.w, a.w, p.w, s.w, decay, xi);
            *(float4*)(t.importance + i) = w;
        } else {
            for (long long j = i; j < t.n; ++j) one(j);
        }
    }
}

// ------------------------------------------------------------------------------------------------ gradient norm and clip coefficient
// Clipping by the global norm without a second pass over the gradients: one pass reads every gradient once (4 B / parameter) and leaves one
// sum of squares per job, the finalize kernel turns them into the norm, torch.nn.utils.clip_grad_norm_'s coefficient and a second hyper
// buffer whose slot 4 is grad_scale * coefficient; the unchanged step kernels are then launched on that buffer.
struct GradTensor { const float* g; long long n; int first_chunk; int nchunks; };
static_assert(sizeof(GradTensor) == 24, "the host side builds 24-byte rows");

// partials[block] = the sum of g[i]^2 over this job's chunk.  The chunk is shifted by the gradient's own `head` as in sgd_chunk (chunk 0
// peels it), the last partial group goes element-wise into the lanes of a zeroed vector, and a lane issues all its loads before the first
// use.  No float atomics: a lane's squares in index order, the shuffle tree, then the four waves in a fixed order, as block_sums.
__global__ void __launch_bounds__(256) grad_sqnorm_kernel(const GradTensor* __restrict__ tensors, const AdamChunk* __restrict__ chunks,
                                                          float* __restrict__ partials) {
    constexpr int GROUPS = ADAM_CHUNK / 1024;
    __shared__ float wsum[4];
    const AdamChunk c = chunks[blockIdx.x];
    const GradTensor t = tensors[c.tensor];
    const int head = chunk_head(t.g);
    float h = 0.f;
    if (c.chunk == 0 && (int)threadIdx.x < head && (long long)threadIdx.x < t.n) h = t.g[threadIdx.x];
    const long long base = (long long)c.chunk * ADAM_CHUNK + head;
    f32x4_a4 g[GROUPS];
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        const long long i = base + 4 * (k * 256 + (int)threadIdx.x);
        if (i + 4 <= t.n) {
            g[k] = *(const f32x4_a4*)(t.g + i);
        } else {
            g[k] = f32x4_a4{0.f, 0.f, 0.f, 0.f};
            if (i < t.n) g[k].x = t.g[i];
            if (i + 1 < t.n) g[k].y = t.g[i + 1];
            if (i + 2 < t.n) g[k].z = t.g[i + 2];
        }
    }
    float s = h * h;
#pragma unroll
    for (int k = 0; k < GROUPS; ++k) {
        s += g[k].x * g[k].x;
        s += g[k].y * g[k].y;
        s += g[k].z * g[k].z;
        s += g[k].w * g[k].w;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One workgroup of CLIP_WAVES waves.  Wave w takes tensors w, w + CLIP_WAVES, ...: lane l adds the tensor's partials l, l + 64, ... in fp64,
// the shuffle tree gives the tensor's sum, and the wave adds its tensors' sums in that order; thread 0 then adds the waves' totals pairwise
// in a fixed tree.  clip_out: [0] norm = sqrt(total) * |grad_scale|, [1] coef = min(1, max_norm / (norm + 1e-6)) with NaN kept (fmin would
// return 1), [2] fp32(grad_scale) * coef, [3] 1 when the norm is not finite; hyper_eff = hyper with slot 4 = clip_out[2].
constexpr int CLIP_WAVES = 16;
__global__ void __launch_bounds__(64 * CLIP_WAVES) grad_clip_final_kernel(const GradTensor* __restrict__ tensors, int ntensors,
                                                                          const float* __restrict__ partials, int nchunks,
                                                                          const float* __restrict__ hyper, double max_norm,
                                                                          float* __restrict__ clip_out, float* __restrict__ tensor_norms,
                                                                          float* __restrict__ hyper_eff) {
    __shared__ double wtot[CLIP_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float gsf = hyper[4];
    const double gs = fabs((double)gsf);
    double total = 0.0;
    for (int ti = wave; ti < ntensors; ti += CLIP_WAVES) {
        const GradTensor t = tensors[ti];
        const int first = t.first_chunk < 0 ? 0 : t.first_chunk;
        const int end = t.first_chunk + t.nchunks < nchunks ? t.first_chunk + t.nchunks : nchunks;      // never past the partials
        double s = 0.0;
        for (int i = first + lane; i < end; i += 64) s += (double)partials[i];
        s = wave_sum_f64(s);
        if (lane == 0 && tensor_norms) tensor_norms[ti] = (float)(sqrt(s) * gs);
        total += s;
    }
    if (lane == 0) wtot[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int o = CLIP_WAVES / 2; o > 0; o >>= 1)
            for (int i = 0; i < o; ++i) wtot[i] += wtot[i + o];
        const double norm = sqrt(wtot[0]) * gs;
        double c = max_norm / (norm + 1e-6);
        c = c > 1.0 ? 1.0 : c;                  // NaN stays NaN
        const float coef = (float)c;
        const float eff = gsf * coef;
        clip_out[0] = (float)norm;
        clip_out[1] = coef;
        clip_out[2] = eff;
        clip_out[3] = isfinite(norm) ? 0.f : 1.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) hyper_eff[j] = j == 4 ? eff : hyper[j];
    }
}

}  // namespace clamd

using namespace clamd;

// The checks every entry point of this file starts with; `who` prefixes the recorded message.
static int check_jobs(const char* who, const void* tensors_dev, const void* chunks_dev, int nchunks) {
    const char* what = nchunks <= 0 ? "no chunks" : (!tensors_dev || !chunks_dev) ? "null tensor or chunk table" : nullptr;
    if (!what) return 0;
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return clamd_fail(msg);
}

static void launch_partial_sum(float* accum, int n, hipStream_t s) {
    hipLaunchKernelGGL(adam_l2_final_kernel, dim3(1), dim3(256), 0, s, accum, n);
}

// the three Adam entry points: importance_dev and path_dev select the instantiation
template <bool EWC, bool TRACK>
static void launch_adam_kernel(const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev, int nchunks,
                               const float* hyper_dev, float* derived_dev, float* ewc_accum_dev, float* l2_accum_dev, hipStream_t s) {
    hipLaunchKernelGGL((adam_kernel<EWC, TRACK>), dim3(nchunks), dim3(256), 0, s, (const AdamTensor*)tensors_dev,
                       (const float* const*)importance_dev, (float* const*)path_dev, (const AdamChunk*)chunks_dev, hyper_dev, derived_dev,
                       ewc_accum_dev, l2_accum_dev);
}

static int launch_adam(const char* what, const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev,
                       int nchunks, const float* hyper_dev, int* step_dev, float* derived_dev, float* ewc_accum_dev, float* l2_accum_dev,
                       void* stream) {
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, s, hyper_dev, step_dev, derived_dev);
    auto launch = importance_dev ? (path_dev ? launch_adam_kernel<true, true> : launch_adam_kernel<true, false>)
                                 : (path_dev ? launch_adam_kernel<false, true> : launch_adam_kernel<false, false>);
    launch(tensors_dev, importance_dev, path_dev, chunks_dev, nchunks, hyper_dev, derived_dev, importance_dev ? ewc_accum_dev : nullptr,
           l2_accum_dev, s);
    if (importance_dev) launch_partial_sum(ewc_accum_dev, nchunks, s);
    if (l2_accum_dev) launch_partial_sum(l2_accum_dev, nchunks, s);
    return clamd_check_launch(what);
}

// both SGD entry points, after their checks
template <bool EWC, bool TRACK>
static void launch_sgd_kernel(const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev, int nchunks,
                              const float* hyper_dev, float* ewc_accum_dev, float* l2_accum_dev, hipStream_t s) {
    hipLaunchKernelGGL((sgd_kernel<EWC, TRACK>), dim3(nchunks), dim3(256), 0, s, (const SgdTensor*)tensors_dev,
                       (const float* const*)importance_dev, (float* const*)path_dev, (const AdamChunk*)chunks_dev, hyper_dev, ewc_accum_dev,
                       l2_accum_dev);
}

static int launch_sgd(const char* what, const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev,
                      int nchunks, const float* hyper_dev, float* ewc_accum_dev, float* l2_accum_dev, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    auto launch = importance_dev ? (path_dev ? launch_sgd_kernel<true, true> : launch_sgd_kernel<true, false>)
                                 : (path_dev ? launch_sgd_kernel<false, true> : launch_sgd_kernel<false, false>);
    launch(tensors_dev, importance_dev, path_dev, chunks_dev, nchunks, hyper_dev, importance_dev ? ewc_accum_dev : nullptr, l2_accum_dev, s);
    if (importance_dev) launch_partial_sum(ewc_accum_dev, nchunks, s);
    if (l2_accum_dev) launch_partial_sum(l2_accum_dev, nchunks, s);
    return clamd_check_launch(what);
}

// the checks of the two SGD entry points behind check_jobs
static int check_sgd(const char* who, const float* hyper_dev, const void* importance_dev, const float* ewc_accum_dev) {
    const char* what = !hyper_dev ? "null hyper buffer"
                       : (importance_dev && !ewc_accum_dev) ? "an importance table needs a penalty buffer (1 + nchunks floats)"
                       : (!importance_dev && ewc_accum_dev) ? "a consolidation penalty buffer without an importance table" : nullptr;
    if (!what) return 0;
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return clamd_fail(msg);
}

extern "C" {

int clamd_sizeof_adam_tensor(void) { return (int)sizeof(AdamTensor); }
int clamd_adam_chunk_elems(void) { return ADAM_CHUNK; }
int clamd_sizeof_importance_tensor(void) { return (int)sizeof(ImportanceTensor); }
int clamd_sizeof_sgd_tensor(void) { return (int)sizeof(SgdTensor); }

int clamd_adam_step(const void* tensors_dev, const void* chunks_dev, int nchunks, const float* hyper_dev, int* step_dev,
                    float* derived_dev, float* l2_accum_dev, void* stream) {
    if (int e = check_jobs("adam", tensors_dev, chunks_dev, nchunks)) return e;
    if (!hyper_dev || !step_dev || !derived_dev) return clamd_fail("adam: null hyper / step / derived buffer");
    return launch_adam("adam_step", tensors_dev, nullptr, nullptr, chunks_dev, nchunks, hyper_dev, step_dev, derived_dev, nullptr, l2_accum_dev,
                       stream);
}

int clamd_adam_step_consolidated(const void* tensors_dev, const void* importance_dev, const void* chunks_dev, int nchunks,
                                 const float* hyper_dev, int* step_dev, float* derived_dev, float* ewc_accum_dev, float* l2_accum_dev,
                                 void* stream) {
    if (int e = check_jobs("adam_step_consolidated", tensors_dev, chunks_dev, nchunks)) return e;
    if (!importance_dev) return clamd_fail("adam_step_consolidated: null importance table");
    if (!hyper_dev || !step_dev || !derived_dev) return clamd_fail("adam_step_consolidated: null hyper / step / derived buffer");
    if (!ewc_accum_dev) return clamd_fail("adam_step_consolidated: null penalty buffer (1 + nchunks floats)");
    return launch_adam("adam_step_consolidated", tensors_dev, importance_dev, nullptr, chunks_dev, nchunks, hyper_dev, step_dev, derived_dev,
                       ewc_accum_dev, l2_accum_dev, stream);
}

int clamd_adam_step_tracked(const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev, int nchunks,
                            const float* hyper_dev, int* step_dev, float* derived_dev, float* ewc_accum_dev, float* l2_accum_dev,
                            void* stream) {
    if (int e = check_jobs("adam_step_tracked", tensors_dev, chunks_dev, nchunks)) return e;
    if (!path_dev) return clamd_fail("adam_step_tracked: null path table");
    if (!hyper_dev || !step_dev || !derived_dev) return clamd_fail("adam_step_tracked: null hyper / step / derived buffer");
    if (importance_dev && !ewc_accum_dev)
        return clamd_fail("adam_step_tracked: an importance table needs a penalty buffer (1 + nchunks floats)");
    if (!importance_dev && ewc_accum_dev) return clamd_fail("adam_step_tracked: a consolidation penalty buffer without an importance table");
    return launch_adam("adam_step_tracked", tensors_dev, importance_dev, path_dev, chunks_dev, nchunks, hyper_dev, step_dev, derived_dev,
                       ewc_accum_dev, l2_accum_dev, stream);
}

int clamd_sgd_step(const void* tensors_dev, const void* importance_dev, const void* chunks_dev, int nchunks, const float* hyper_dev,
                   float* ewc_accum_dev, float* l2_accum_dev, void* stream) {
    if (int e = check_jobs("sgd_step", tensors_dev, chunks_dev, nchunks)) return e;
    if (int e = check_sgd("sgd_step", hyper_dev, importance_dev, ewc_accum_dev)) return e;
    return launch_sgd("sgd_step", tensors_dev, importance_dev, nullptr, chunks_dev, nchunks, hyper_dev, ewc_accum_dev, l2_accum_dev, stream);
}

int clamd_sgd_step_tracked(const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev, int nchunks,
                           const float* hyper_dev, float* ewc_accum_dev, float* l2_accum_dev, void* stream) {
    if (int e = check_jobs("sgd_step_tracked", tensors_dev, chunks_dev, nchunks)) return e;
    if (!path_dev) return clamd_fail("sgd_step_tracked: null path table");
    if (int e = check_sgd("sgd_step_tracked", hyper_dev, importance_dev, ewc_accum_dev)) return e;
    return launch_sgd("sgd_step_tracked", tensors_dev, importance_dev, path_dev, chunks_dev, nchunks, hyper_dev, ewc_accum_dev, l2_accum_dev,
                      stream);
}

int clamd_sizeof_path_tensor(void) { return (int)sizeof(PathTensor); }

int clamd_path_importance(const void* tensors_dev, const void* chunks_dev, int nchunks, double decay, double xi, void* stream) {
    if (int e = check_jobs("path_importance", tensors_dev, chunks_dev, nchunks)) return e;
    if (!(decay >= 0.0) || !(decay <= 3.0e38)) return clamd_fail("path_importance: decay must be finite and >= 0");
    if (!(xi > 0.0) || !(xi <= 3.0e38) || !((float)xi > 0.f)) return clamd_fail("path_importance: xi must be finite and > 0 (in fp32)");
    hipLaunchKernelGGL(path_importance_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, (const PathTensor*)tensors_dev,
                       (const AdamChunk*)chunks_dev, (float)decay, (float)xi);
    return clamd_check_launch("path_importance");
}

int clamd_importance_accum(const void* tensors_dev, const void* chunks_dev, int nchunks, double decay, double scale, int power, void* stream) {
    if (int e = check_jobs("importance_accum", tensors_dev, chunks_dev, nchunks)) return e;
    if (power != 1 && power != 2) return clamd_fail("importance_accum: power must be 1 or 2");
    if (!(decay >= 0.0) || !(decay <= 3.0e38)) return clamd_fail("importance_accum: decay must be finite and >= 0");
    if (!(scale >= 0.0) || !(scale <= 3.0e38)) return clamd_fail("importance_accum: scale must be finite and >= 0");
    hipStream_t s = (hipStream_t)stream;
    if (power == 2)
        hipLaunchKernelGGL(importance_accum_kernel<true>, dim3(nchunks), dim3(256), 0, s, (const ImportanceTensor*)tensors_dev,
                           (const AdamChunk*)chunks_dev, (float)decay, (float)scale);
    else
        hipLaunchKernelGGL(importance_accum_kernel<false>, dim3(nchunks), dim3(256), 0, s, (const ImportanceTensor*)tensors_dev,
                           (const AdamChunk*)chunks_dev, (float)decay, (float)scale);
    return clamd_check_launch("importance_accum");
}

int clamd_sizeof_grad_tensor(void) { return (int)sizeof(GradTensor); }

int clamd_grad_norm_clip(const void* tensors_dev, int ntensors, const void* chunks_dev, int nchunks, const float* hyper_dev, double max_norm,
                         float* partials, float* clip_out, float* tensor_norms, float* hyper_eff, void* stream) {
    if (int e = check_jobs("grad_norm_clip", tensors_dev, chunks_dev, nchunks)) return e;
    if (ntensors <= 0) return clamd_fail("grad_norm_clip: no tensors");
    if (!hyper_dev || !partials || !clip_out || !hyper_eff) return clamd_fail("grad_norm_clip: null hyper / partials / clip_out / hyper_eff buffer");
    if (!(max_norm > 0.0)) return clamd_fail("grad_norm_clip: max_norm must be > 0 (infinity: measure only)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(nchunks), dim3(256), 0, s, (const GradTensor*)tensors_dev, (const AdamChunk*)chunks_dev, partials);
    hipLaunchKernelGGL(grad_clip_final_kernel, dim3(1), dim3(64 * CLIP_WAVES), 0, s, (const GradTensor*)tensors_dev, ntensors, partials, nchunks,
                       hyper_dev, max_norm, clip_out, tensor_norms, hyper_eff);
    return clamd_check_launch("grad_norm_clip");
}

}  // extern "C"
