// Local POD distillation (build-defined, parity unpinned: the reference has no continual-learning code; the distillation half of PLOP,
// Douillard et al., CVPR 2021, section 3.1, as include/clamd.h restates it): multi-scale strip-pooled statistics of a new tensor matched to
// an old one's.  clamd_local_pod_fwd_bwd enqueues four launches:
//   pod_strip_kernel<NPX>     one pass over a and b: the finest level's unnormalised row sums per column slot (R) and column sums per row
//                             band (Q); the background merge and the squaring happen here
//   pod_finalize_kernel<L>    per image, fp64 in a fixed order: coarser levels from the finest sums, the norms, the distance (from the
//                             differences), the normalisation Jacobian's dot product, and the coefficient tables Grow / Gcol
//   pod_loss_kernel           loss = lam / B * sum_n dist_n, ascending n
//   pod_grad_kernel<NPX>      da = (Grow + Gcol) * (square ? 2 * value : 1) over all Ca channels (skipped when da == NULL)
// No atomics, every buffer element written whole with plain stores: bit-reproducible.  NPX = 4 is the 16-byte form (W % 4 == 0, 16-byte
// aligned bases), NPX = 1 the same arithmetic for any other width or alignment.
#include <math.h>
#include <stdio.h>
#include "common.hip.h"
#include "clamd_internal.h"

namespace clamd {

// How the strip pass lays a row's partial sums out.  A finest-level column segment is wf = W / kmax pixels wide.  Grouped form (g > 0):
// wf is a whole number of lanes (wf = NPX * l) with l a power of two <= 64 or a multiple of 64; g = min(l, 64) neighbouring lanes add
// their sums with log2(g) shuffles and the group's first lane stores slot x / (NPX * g): nslots = W / (NPX * g), a segment is
// nslots / kmax consecutive slots.  General form (g == 0, any other width): every wave reduces one value per segment over its 64 lanes,
// slot = wave_chunk * kmax + segment: nslots = ceil(W / (64 * NPX)) * kmax, a segment is every kmax-th slot.
static void pod_slots(int W, int kmax, int npx, int* g, int* nslots) {
    const int wf = W / kmax;
    if (wf % npx == 0) {
        const int l = wf / npx;
        if (l <= 64 && (l & (l - 1)) == 0) { *g = l; *nslots = kmax; return; }
        if (l % 64 == 0) { *g = 64; *nslots = W / (npx * 64); return; }
    }
    *g = 0;
    *nslots = (W + 64 * npx - 1) / (64 * npx) * kmax;
}

template <int NPX>
__device__ inline void pod_ld(const float* __restrict__ p, float (&v)[NPX]) {
    if constexpr (NPX == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int NPX>
__device__ inline void pod_st(float* __restrict__ p, const float (&v)[NPX]) {
    if constexpr (NPX == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// A workgroup owns (row band, compared channel, image and tensor): grid (nb, C, 2 B), blockIdx.z = 2 n + (0: a, 1: b).  It walks the
// band's hb rows in ascending order, 256 * NPX columns at a time (one trip for W <= 1024 in the 16-byte form), the per-column sums in
// registers.  Channel 0 of a under merge_extra is a_0 + a_C + ... + a_{Ca-1}, added in that order.
template <int NPX>
__global__ void __launch_bounds__(256) pod_strip_kernel(const float* __restrict__ a, const float* __restrict__ b, int Ca, int Cb, int C,
                                                        int merge, int square, int H, int W, int nb, int hb, int kmax, int g, int nslots,
                                                        float* __restrict__ R, long long r_each, float* __restrict__ Q, long long q_each) {
    const int band = blockIdx.x, c = blockIdx.y, n = blockIdx.z >> 1, which = blockIdx.z & 1;
    const float* __restrict__ src = which ? b : a;
    const int Cs = which ? Cb : Ca;
    const int nextra = (!which && merge && c == 0) ? Ca - C : 0;
    const long long HW = (long long)H * W;
    const float* __restrict__ plane = src + ((long long)n * Cs + c) * HW;
    const float* __restrict__ extra = src + ((long long)n * Cs + C) * HW;
    float* __restrict__ Rout = R + which * r_each + ((long long)n * C + c) * H * nslots;
    float* __restrict__ Qout = Q + which * q_each + (((long long)n * C + c) * nb + band) * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wf = W / kmax, y0 = band * hb;
    for (int col0 = 0; col0 < W; col0 += 256 * NPX) {
        const int wave_col = col0 + wave * 64 * NPX;
        if (wave_col >= W) break;                               // wave-uniform; later trips start further right
        const int x = wave_col + lane * NPX;
        const bool live = x < W;                                // W % NPX == 0: a live lane's NPX columns are all inside
        int sg[NPX];
#pragma unroll
        for (int i = 0; i < NPX; ++i) sg[i] = (x + i) / wf;
        float cs[NPX];
#pragma unroll
        for (int i = 0; i < NPX; ++i) cs[i] = 0.f;
        for (int y = y0; y < y0 + hb; ++y) {
            float v[NPX];
#pragma unroll
            for (int i = 0; i < NPX; ++i) v[i] = 0.f;
            if (live) {
                const long long o = (long long)y * W + x;
                pod_ld<NPX>(plane + o, v);
                for (int k = 0; k < nextra; ++k) {
                    float e[NPX];
                    pod_ld<NPX>(extra + k * HW + o, e);
#pragma unroll
                    for (int i = 0; i < NPX; ++i) v[i] += e[i];
                }
                if (square) {
#pragma unroll
                    for (int i = 0; i < NPX; ++i) v[i] *= v[i];
                }
            }
#pragma unroll
            for (int i = 0; i < NPX; ++i) cs[i] += v[i];
            if (g) {                                            // the lane's NPX columns lie in one segment
                float s;
                if constexpr (NPX == 4) s = (v[0] + v[1]) + (v[2] + v[3]);
                else s = v[0];
                for (int o = 1; o < g; o <<= 1) s += __shfl_xor(s, o);
                if (live && (lane & (g - 1)) == 0) Rout[(long long)y * nslots + x / (NPX * g)] = s;
            } else {
                const int wc = wave_col / (64 * NPX);
                for (int j = 0; j < kmax; ++j) {
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < NPX; ++i) s += sg[i] == j ? v[i] : 0.f;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
                    if (lane == 0) Rout[(long long)y * nslots + wc * kmax + j] = s;
                }
            }
        }
        if (live) pod_st<NPX>(Qout + x, cs);
    }
}

struct PodFin {
    const float *Ra, *Rb, *Qa, *Qb;
    float *Grow, *Gcol;
    double* dist;
    int C, H, W, nb, nslots, general, normalize;
    double scale;              // lam / B * grad_scale
};

// sum of 256 per-thread values in a fixed tree; every thread gets the result
__device__ inline double pod_block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// The embedding entries of one item, both tensors: a row item (c, y) holds r[s, c, y, :], a column item (c, x) q[s, c, :, x], every
// level s, entry (1 << s) - 1 + j for region j.  The finest sums come from the strip pass's slots / bands in ascending order, the
// coarser levels are pairwise sums of the finer ones.  -> the item's offset into Grow (row) or Gcol (column) and the stride between
// two finest regions there.
template <int L>
__device__ inline void pod_item(const PodFin& p, int n, long long idx, double (&ea)[(1 << L) - 1], double (&eb)[(1 << L) - 1],
                                double (&inv)[L], bool* row, long long* gofs, long long* gstride) {
    constexpr int KM = 1 << (L - 1);
    double fa[KM], fb[KM];
    const long long rows = (long long)p.C * p.H;
    *row = idx < rows;
    if (*row) {
        const long long base = ((long long)n * rows + idx) * p.nslots;
        const int per = p.nslots / KM, stride = p.general ? KM : 1;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            const int first = p.general ? j : j * per;
            double sa = 0.0, sb = 0.0;
            for (int t = 0; t < per; ++t) {
                sa += (double)p.Ra[base + first + t * stride];
                sb += (double)p.Rb[base + first + t * stride];
            }
            fa[j] = sa; fb[j] = sb;
        }
#pragma unroll
        for (int s = 0; s < L; ++s) inv[s] = 1.0 / (double)(p.W >> s);
        *gofs = ((long long)n * rows + idx) * KM;
        *gstride = 1;
    } else {
        const long long i2 = idx - rows;
        const int c = (int)(i2 / p.W), x = (int)(i2 - (long long)c * p.W);
        const int per = p.nb / KM;
        const long long base = ((long long)n * p.C + c) * p.nb * p.W + x;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            double sa = 0.0, sb = 0.0;
            for (int t = 0; t < per; ++t) {
                sa += (double)p.Qa[base + (long long)(j * per + t) * p.W];
                sb += (double)p.Qb[base + (long long)(j * per + t) * p.W];
            }
            fa[j] = sa; fb[j] = sb;
        }
#pragma unroll
        for (int s = 0; s < L; ++s) inv[s] = 1.0 / (double)(p.H >> s);
        *gofs = ((long long)n * p.C + c) * KM * p.W + x;
        *gstride = p.W;
    }
#pragma unroll
    for (int s = L - 1; s >= 0; --s) {
#pragma unroll
        for (int j = 0; j < (1 << s); ++j) {
            ea[(1 << s) - 1 + j] = fa[j] * inv[s];
            eb[(1 << s) - 1 + j] = fb[j] * inv[s];
        }
#pragma unroll
        for (int j = 0; j < (1 << s) / 2; ++j) {
            fa[j] = fa[2 * j] + fa[2 * j + 1];
            fb[j] = fb[2 * j] + fb[2 * j + 1];
        }
    }
}

// One workgroup per image; the C (H + W) items are dealt to the 256 threads round robin, so every per-thread sum and the tree over the
// threads have a fixed order.  Three walks over the (L2-resident) sums: the norms; the distance and e_a . d; the tables.
//   e = emb * i,  i = 1 / max(||emb||, 1e-12) (1 without normalize);  d = e_a - e_b;  dist = ||d||;  u = d / dist (0 when dist == 0)
//   d dist / d emb_a = (u - e_a (e_a . u)) * i_a   (normalised, ||emb_a|| > 1e-12);  u * 1e12 (normalised, below the clamp);  u (not normalised)
//   Grow[n, c, y, j] = scale * sum_s (1 / w_s) * that at r[s, c, y, j >> (L-1-s)],  Gcol likewise with 1 / h_s and q.
template <int L>
__global__ void __launch_bounds__(256) pod_finalize_kernel(PodFin p) {
#pragma clang fp contract(off)      // e_a - e_b from two rounded products (no fma): identical tensors give exactly 0
    constexpr int KM = 1 << (L - 1), NV = (1 << L) - 1;
    __shared__ double sh[256];
    const int n = blockIdx.x;
    const long long items = (long long)p.C * (p.H + p.W);
    double ea[NV], eb[NV], inv[L];
    bool row;
    long long gofs, gstride;
    double ia = 1.0, ib = 1.0, ja = 1.0;
    bool project = false;
    if (p.normalize) {
        double na = 0.0, nbb = 0.0;
        for (long long i = threadIdx.x; i < items; i += 256) {
            pod_item<L>(p, n, i, ea, eb, inv, &row, &gofs, &gstride);
#pragma unroll
            for (int k = 0; k < NV; ++k) { na += ea[k] * ea[k]; nbb += eb[k] * eb[k]; }
        }
        na = sqrt(pod_block_sum(na, sh));
        nbb = sqrt(pod_block_sum(nbb, sh));
        project = na > 1e-12;
        ia = 1.0 / fmax(na, 1e-12);
        ib = 1.0 / fmax(nbb, 1e-12);
        ja = ia;
    }
    double d2 = 0.0, pd = 0.0;
    for (long long i = threadIdx.x; i < items; i += 256) {
        pod_item<L>(p, n, i, ea, eb, inv, &row, &gofs, &gstride);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const double e = ea[k] * ia, d = e - eb[k] * ib;
            d2 += d * d;
            pd += e * d;
        }
    }
    const double dist = sqrt(pod_block_sum(d2, sh));
    pd = pod_block_sum(pd, sh);
    if (threadIdx.x == 0) p.dist[n] = dist;
    const double idist = dist > 0.0 ? 1.0 / dist : 0.0;
    const double proj = project ? pd * idist : 0.0, coef = p.scale * ja;
    for (long long i = threadIdx.x; i < items; i += 256) {
        pod_item<L>(p, n, i, ea, eb, inv, &row, &gofs, &gstride);
        double ge[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const double e = ea[k] * ia, d = e - eb[k] * ib;
            ge[k] = coef * (d * idist - e * proj);
        }
        float* __restrict__ out = (row ? p.Grow : p.Gcol) + gofs;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            double t = 0.0;
#pragma unroll
            for (int s = 0; s < L; ++s) t += ge[(1 << s) - 1 + (j >> (L - 1 - s))] * inv[s];
            out[j * gstride] = (float)t;
        }
    }
}

__global__ void pod_loss_kernel(const double* __restrict__ dist, float* __restrict__ loss1, double lam_over_b, int B) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int n = 0; n < B; ++n) s += dist[n];
        loss1[0] = (float)(lam_over_b * s);
    }
}

// grid (ceil(H W / NPX / 256), C, B): a thread owns NPX consecutive pixels of one compared channel and writes them; the threads of
// channel 0 also write the channels >= C (channel 0's gradient under merge_extra, zeros otherwise).  a is read only when square is set.
template <int NPX>
__global__ void __launch_bounds__(256) pod_grad_kernel(const float* __restrict__ a, const float* __restrict__ Grow, const float* __restrict__ Gcol,
                                                       float* __restrict__ da, int Ca, int C, int merge, int square, int H, int W, int kmax) {
    const long long HW = (long long)H * W, pix = ((long long)blockIdx.x * 256 + threadIdx.x) * NPX;
    if (pix >= HW) return;
    const int c = blockIdx.y, n = blockIdx.z, y = (int)(pix / W), x = (int)(pix - (long long)y * W), wf = W / kmax, hf = H / kmax;
    float val[NPX];
    pod_ld<NPX>(Gcol + (((long long)n * C + c) * kmax + y / hf) * W + x, val);
    const float* __restrict__ gr = Grow + (((long long)n * C + c) * H + y) * kmax;
#pragma unroll
    for (int i = 0; i < NPX; ++i) val[i] = gr[(x + i) / wf] + val[i];
    const long long image = (long long)n * Ca * HW;
    const int nextra = c == 0 ? Ca - C : 0;
    if (square) {
        float m[NPX];
        pod_ld<NPX>(a + image + c * HW + pix, m);
        if (merge)
            for (int k = 0; k < nextra; ++k) {
                float e[NPX];
                pod_ld<NPX>(a + image + (C + k) * HW + pix, e);
#pragma unroll
                for (int i = 0; i < NPX; ++i) m[i] += e[i];
            }
#pragma unroll
        for (int i = 0; i < NPX; ++i) val[i] *= 2.f * m[i];
    }
    pod_st<NPX>(da + image + c * HW + pix, val);
    if (nextra) {
        if (!merge) {
#pragma unroll
            for (int i = 0; i < NPX; ++i) val[i] = 0.f;
        }
        for (int k = 0; k < nextra; ++k) pod_st<NPX>(da + image + (C + k) * HW + pix, val);
    }
}

}  // namespace clamd

using namespace clamd;

// The workspace, in floats from a 16-byte aligned base, every part starting on 16 bytes: Ra, Rb [B][C][H][nslots]; Qa, Qb [B][C][nb][W];
// Grow [B][C][H][kmax]; Gcol [B][C][kmax][W]; dist: B doubles.  R is sized for the wider of the two access forms.  nb row bands per
// (image, channel): kmax times a power of two that divides H / kmax, doubled while a band keeps >= 8 rows and the grid has fewer than
// 1024 workgroups -- a function of the shape alone.
struct PodLayout {
    int kmax, nb, hb;
    long long r_each, q_each, grow, gcol;       // floats
    long long o_rb, o_qa, o_qb, o_grow, o_gcol, o_dist, total;
};

static long long pod_up4(long long v) { return (v + 3) & ~3ll; }

static bool pod_layout(int B, int C, int H, int W, int levels, PodLayout* l) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || levels < 1 || levels > 3) return false;
    const int kmax = 1 << (levels - 1);
    if (H % kmax || W % kmax) return false;
    int m = 1;
    const int rows = H / kmax;
    while (rows % (2 * m) == 0 && rows / (2 * m) >= 8 && 2ll * B * C * kmax * m < 1024) m *= 2;
    int g4, s4 = 0, g1, s1;
    pod_slots(W, kmax, 1, &g1, &s1);
    if (W % 4 == 0) pod_slots(W, kmax, 4, &g4, &s4);
    l->kmax = kmax; l->nb = kmax * m; l->hb = H / l->nb;
    const long long bc = (long long)B * C;
    l->r_each = pod_up4(bc * H * (s1 > s4 ? s1 : s4));
    l->q_each = pod_up4(bc * l->nb * W);
    l->grow = pod_up4(bc * H * kmax);
    l->gcol = pod_up4(bc * kmax * W);
    l->o_rb = l->r_each;
    l->o_qa = 2 * l->r_each;
    l->o_qb = l->o_qa + l->q_each;
    l->o_grow = l->o_qb + l->q_each;
    l->o_gcol = l->o_grow + l->grow;
    l->o_dist = l->o_gcol + l->gcol;
    l->total = l->o_dist + pod_up4(2ll * B);
    return true;
}

extern "C" {

size_t clamd_pod_workspace_bytes(int B, int C, int H, int W, int levels) {
    PodLayout l;
    return pod_layout(B, C, H, W, levels, &l) ? (size_t)l.total * sizeof(float) : 0;
}

int clamd_local_pod_fwd_bwd(const float* a, int Ca, const float* b, int Cb, int C, int merge_extra, int square, int normalize, int levels,
                            double lam, float* da, float* loss1, void* workspace, size_t ws_bytes, int B, int H, int W, double grad_scale,
                            void* stream) {
    if (!a || !b || !loss1 || !workspace || B <= 0 || H <= 0 || W <= 0 || Ca <= 0 || Cb <= 0)
        return clamd_fail("local_pod_fwd_bwd: null pointer or empty shape");
    if (levels < 1 || levels > 3) return clamd_fail("local_pod_fwd_bwd: levels must be 1, 2 or 3");
    if (C < 1 || C > Ca || C > Cb) return clamd_fail("local_pod_fwd_bwd: C must be in [1, min(Ca, Cb)]");
    PodLayout l;
    if (!pod_layout(B, C, H, W, levels, &l)) return clamd_fail("local_pod_fwd_bwd: H and W must be multiples of 2^(levels-1)");
    if (B > 32767 || C > 65535) return clamd_fail("local_pod_fwd_bwd: at most 32767 images and 65535 compared channels per call");
    if (!(fabs(lam) <= 3.0e38) || !(fabs(grad_scale) <= 3.0e38)) return clamd_fail("local_pod_fwd_bwd: lam and grad_scale must be finite");
    if (((size_t)a % 4) || ((size_t)b % 4) || ((size_t)da % 4) || ((size_t)loss1 % 4) || ((size_t)workspace % 16))
        return clamd_fail("local_pod_fwd_bwd: misaligned tensor (fp32 tensors 4 bytes, the workspace 16)");
    if (ws_bytes < (size_t)l.total * sizeof(float)) return clamd_fail("local_pod_fwd_bwd: workspace smaller than clamd_pod_workspace_bytes");
    float* ws = (float*)workspace;
    const bool four = W % 4 == 0 && ((size_t)a % 16) == 0 && ((size_t)b % 16) == 0;
    int g, nslots;
    pod_slots(W, l.kmax, four ? 4 : 1, &g, &nslots);
    hipStream_t s = (hipStream_t)stream;
    const dim3 sgrid(l.nb, C, 2 * B);
#define POD_STRIP(NPX_) hipLaunchKernelGGL((pod_strip_kernel<NPX_>), sgrid, dim3(256), 0, s, a, b, Ca, Cb, C, merge_extra ? 1 : 0, square ? 1 : 0, H, W, l.nb, l.hb, l.kmax, g, nslots, ws, l.r_each, ws + l.o_qa, l.q_each)
    if (four) POD_STRIP(4); else POD_STRIP(1);
#undef POD_STRIP
    PodFin p;
    p.Ra = ws; p.Rb = ws + l.o_rb; p.Qa = ws + l.o_qa; p.Qb = ws + l.o_qb;
    p.Grow = ws + l.o_grow; p.Gcol = ws + l.o_gcol; p.dist = (double*)(ws + l.o_dist);
    p.C = C; p.H = H; p.W = W; p.nb = l.nb; p.nslots = nslots; p.general = g == 0; p.normalize = normalize ? 1 : 0;
    p.scale = lam / (double)B * grad_scale;
    if (levels == 1) hipLaunchKernelGGL((pod_finalize_kernel<1>), dim3(B), dim3(256), 0, s, p);
    else if (levels == 2) hipLaunchKernelGGL((pod_finalize_kernel<2>), dim3(B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((pod_finalize_kernel<3>), dim3(B), dim3(256), 0, s, p);
    hipLaunchKernelGGL(pod_loss_kernel, dim3(1), dim3(64), 0, s, p.dist, loss1, lam / (double)B, B);
    if (da) {
        const bool gfour = W % 4 == 0 && ((size_t)da % 16) == 0 && (!square || ((size_t)a % 16) == 0);
        const long long quads = ((long long)H * W) / (gfour ? 4 : 1);
        const dim3 ggrid((unsigned int)((quads + 255) / 256), C, B);
#define POD_GRAD(NPX_) hipLaunchKernelGGL((pod_grad_kernel<NPX_>), ggrid, dim3(256), 0, s, a, p.Grow, p.Gcol, da, Ca, C, merge_extra ? 1 : 0, square ? 1 : 0, H, W, l.kmax)
        if (gfour) POD_GRAD(4); else POD_GRAD(1);
#undef POD_GRAD
    }
    return clamd_check_launch("local_pod_fwd_bwd");
}

}  // extern "C"
